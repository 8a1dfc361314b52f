"""ga_fr_lagrange_at, ga_fr_sparse_matvec, ga_fr_compact_nonzero, ga_fr_powers and g16_setup.Setup on a real MI355X: the cases of
tests/test_setup_scalars.py through the hipcc-built library, sizes beyond one workgroup, one capped grid and one scan tile, and Setup at
2^12 constraints followed by MSMs over the device-resident key."""
import numpy as np
import pytest

import oracle
import pyref
import test_phase2_init as p2
import test_setup_scalars as cases
import test_to_lagrange as tl
from gnark_amd import ecc, g16_setup
from helpers import BLS12_381, BN254, arr_to_fr, fr_to_arr

pytestmark = pytest.mark.gpu
CURVES = [BN254, BLS12_381]


@pytest.mark.parametrize("mont", cases.FORMS, ids=cases.FORM_IDS)
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_lagrange_at(gpu_ctx, c, mont):
    cases.test_lagrange_at(gpu_ctx, c, mont)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_lagrange_at_2_16(gpu_ctx, c, n=1 << 16):
    """n = 2^16, m = 2^16 - 5: sixteen workgroups of the power kernel (4096 indices each, 256 apart inside a lane) and more than one
    block of the batch inversion; 64 sampled indices with 0, m - 1 and both sides of a workgroup and of a lane-step boundary.  m = n:
    sum_i L_i(tau) = 1, through ga_fr_dot against a vector of ones"""
    ctx, lib = gpu_ctx, gpu_ctx.lib
    tau, m = tl.tau_of(c), n - 5
    rng = pyref.Xoshiro(0x1A6A + c.cid)
    idx = sorted({0, 1, 255, 256, 4095, 4096, 4097, 8191, 8192, m - 1} | {rng.next() % m for _ in range(54)})
    want = tl.lagrange_scalars(c, n, tau, idx)
    for mont in cases.FORMS:
        got = g16_setup.LagrangeAt(ctx, c.name, n, tau, m, montgomery=mont)
        assert got.shape == (m, 4) and cases.ints(c, got[idx], mont) == want, mont
    d_lag = g16_setup.LagrangeAt(ctx, c.name, n, tau, montgomery=True, out_device=True)
    d_one = ctx.to_device(fr_to_arr(c, [1] * n, mont=False))
    try:
        dot = np.zeros(4, np.uint64)
        lib.check(lib.ga_fr_dot(ctx.handle, c.cid, d_lag.ptr, d_one.ptr, n, dot.ctypes.data))   # a Montgomery, b canonical -> canonical
        assert arr_to_fr(c, dot, mont=False) == [1]
    finally:
        d_lag.free()
        d_one.free()


@pytest.mark.parametrize("mont", cases.FORMS, ids=cases.FORM_IDS)
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_matvec_coefficient_table(gpu_ctx, c, mont):
    cases.test_matvec_coefficient_table(gpu_ctx, c, mont)


@pytest.mark.parametrize("S", [2, 16])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_matvec_row_lengths(gpu_ctx, monkeypatch, c, S):
    cases.test_matvec_row_lengths(gpu_ctx, monkeypatch, c, S)


@pytest.mark.parametrize("mont", cases.FORMS, ids=cases.FORM_IDS)
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_matvec_row_scales(gpu_ctx, monkeypatch, c, mont):
    cases.test_matvec_row_scales(gpu_ctx, monkeypatch, c, mont)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_matvec_beyond_one_grid(gpu_ctx, c, n_rows=(1 << 18) + 77, n_cols=1 << 12):
    """2^18 + 77 rows of two or three terms over 2^12 x values: more segments than the 1024 workgroups of 256 lanes of a launch hold
    (the grid-stride loop).  The rows on either side of the first stride and the last row word for word, and sum_r z_r out[r] through
    ga_fr_dot over the device-resident output against the Python sum"""
    ctx, lib = gpu_ctx, gpu_ctx.lib
    rng = np.random.default_rng(0x5BA6 + c.cid)

    def rand_words(n):
        w = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        w[:, 3] = rng.integers(1, c.r >> 192, size=n, dtype=np.uint64)   # below r
        return w, [int.from_bytes(row.tobytes(), "little") for row in w]
    (X, x), (Z, z) = rand_words(n_cols), rand_words(n_rows)
    table = p2.coeff_table(c)
    length = rng.integers(2, 4, size=n_rows).astype(np.uint64)
    stride = 1024 * 256
    length[[stride - 1, stride, n_rows - 1]] = 3
    row_start = np.zeros(n_rows + 1, np.uint64)
    row_start[1:] = np.cumsum(length)
    nnz = int(row_start[-1])
    terms = np.stack([rng.integers(0, len(table), size=nnz), rng.integers(0, n_cols, size=nnz)], axis=1).astype(np.uint32)
    prod = [table[cid] * x[col] % c.r for cid, col in terms.tolist()]
    rs = row_start.astype(np.int64).tolist()
    value = [sum(prod[rs[r]:rs[r + 1]]) % c.r for r in range(n_rows)]
    total = sum(v * k for v, k in zip(value, z)) % c.r
    sample = [0, stride - 1, stride, stride + 1, n_rows - 1]
    d_x, d_z = ctx.to_device(fr_to_arr(c, x)), ctx.to_device(Z)
    d_out = None
    try:
        d_out = g16_setup.SparseMatVec(ctx, c.name, d_x, row_start, terms, p2.coeff_arr(c, table, True), montgomery=True, n_cols=n_cols, out_device=True)
        assert arr_to_fr(c, d_out.to_host((n_rows, 4))[sample]) == [value[r] for r in sample]
        dot = np.zeros(4, np.uint64)
        lib.check(lib.ga_fr_dot(ctx.handle, c.cid, d_out.ptr, d_z.ptr, n_rows, dot.ctypes.data))
        assert arr_to_fr(c, dot, mont=False) == [total]
    finally:
        for b in (d_out, d_x, d_z):
            if b is not None:
                b.free()


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_compact_nonzero(gpu_ctx, c):
    cases.test_compact_nonzero(gpu_ctx, c)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_compact_nonzero_2_18(gpu_ctx, c, n=(1 << 18) + 3):
    """n = 2^18 + 3, about 30 % zeros, zeros at both ends: many tiles of the scan; device in, device out and in place"""
    ctx = gpu_ctx
    rng = np.random.default_rng(0xC0A7 + c.cid)
    v = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    v[:, 3] = rng.integers(1, c.r >> 192, size=n, dtype=np.uint64)
    zero = rng.integers(0, 10, size=n) < 3
    zero[[0, n - 1]] = True
    v[zero] = 0
    want = v[~zero]
    d_v = ctx.to_device(v)
    try:
        d_out, mask, count = g16_setup.CompactNonZero(ctx, c.name, d_v, n, out_device=True)
        try:
            assert count == want.shape[0] and np.array_equal(mask, zero)
            assert np.array_equal(d_out.to_host((count, 4)), want) and np.array_equal(d_v.to_host((n, 4)), v)
        finally:
            d_out.free()
        _, mask, count = g16_setup.CompactNonZero(ctx, c.name, d_v, n, in_place=True)
        got = d_v.to_host((n, 4))
        assert count == want.shape[0] and np.array_equal(mask, zero)
        assert np.array_equal(got[:count], want) and np.array_equal(got[count:], v[count:])
    finally:
        d_v.free()


@pytest.mark.parametrize("mont", cases.FORMS, ids=cases.FORM_IDS)
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_powers(gpu_ctx, c, mont):
    cases.test_powers(gpu_ctx, c, mont)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_placement_and_purity(gpu_ctx, c):
    cases.test_placement_and_purity(gpu_ctx, c)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_errors(gpu_ctx, monkeypatch, c):
    cases.test_errors(gpu_ctx, monkeypatch, c)


@pytest.mark.parametrize("mont", cases.FORMS, ids=cases.FORM_IDS)
@pytest.mark.parametrize("circuit", list(p2.CIRCUITS))
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_setup_replay(gpu_ctx, c, circuit, mont):
    cases.test_setup_replay(gpu_ctx, c, circuit, mont)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_setup_then_msm_2_12(gpu_ctx, c, m=1 << 12, n_wires=3000):
    """a random R1CS of 2^12 constraints over 3 000 wires, general alpha .. tau: Setup on the device, then ga_msm over the
    device-resident compacted A with a random witness filtered by infinityA == [sum w_i A_i(tau)]G, and over pk.K and vk.K ==
    [sum w_i kk_i / delta]G and [sum w_i kk_i / gamma]G, from the integers of test_phase2_init.setup_scalars -- no vector of the key
    leaves the device"""
    ctx = gpu_ctx
    cs = p2.random_r1cs(c, m, n_wires, 0x2C13)
    toxic = cases.general_toxic(c, cs, 0x2418)
    alpha, beta, gamma, delta, tau = toxic[:5]
    n, logs = p2.setup_scalars(c, cs, alpha, beta, tau)
    assert n == m
    rng = pyref.Xoshiro(0x2419 + c.cid)
    w = [rng.field(c.r) for _ in range(n_wires)]
    key = g16_setup.Setup(ctx, c.name, cases.setup_matrices(c, cs, True), toxic)
    try:
        assert list(key.infinityA) == [a == 0 for a in logs["A"]] and list(key.infinityB) == [b == 0 for b in logs["B"]]
        assert 0 < key.len_a == sum(1 for a in logs["A"] if a) < n_wires
        assert key.len_k == n_wires - cs.nb_public and key.len_vk == cs.nb_public

        def msm(buf, count, scalars):
            return oracle.jac_to_affine(c.cid, 0, ecc.MultiExp(ctx, c.name, 0, buf, fr_to_arr(c, scalars), n=count))

        def point(k):
            return oracle.jac_to_affine(c.cid, 0, oracle.generator_mul(c.cid, 0, k % c.r))
        keep = [i for i in range(n_wires) if logs["A"][i]]
        assert np.array_equal(msm(key.A, key.len_a, [w[i] for i in keep]), point(sum(w[i] * logs["A"][i] for i in keep)))
        dinv, ginv = pow(delta, -1, c.r), pow(gamma, -1, c.r)
        private = range(cs.nb_public, n_wires)
        assert np.array_equal(msm(key.K, key.len_k, [w[i] for i in private]), point(sum(w[i] * logs["K"][i] for i in private) * dinv))
        public = range(cs.nb_public)
        assert np.array_equal(msm(key.vkK, key.len_vk, [w[i] for i in public]), point(sum(w[i] * logs["K"][i] for i in public) * ginv))
    finally:
        key.free()

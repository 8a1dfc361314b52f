"""ga_sparse_point_sums and ga_lagrange_coeffs on a real MI355X: the cases of tests/test_phase2_init.py through the hipcc-built
library, a matrix beyond one capped grid of every stage, and Phase2.Initialize at 2^12 constraints with an MSM over the device-resident
result."""
import numpy as np
import pytest

import oracle
import pyref
import test_fixed_base as fb
import test_phase2_init as cases
from gnark_amd import ecc
from gnark_amd.device import affine_words
from helpers import BLS12_381, BN254, fr_to_arr

pytestmark = pytest.mark.gpu
CURVES = [BN254, BLS12_381]


@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "montgomery"])
@pytest.mark.parametrize("c,group", cases.PAIRS, ids=cases.PAIR_IDS)
def test_sparse_sums_coefficient_classes(gpu_ctx, c, group, mont):
    cases.test_sparse_sums_coefficient_classes(gpu_ctx, c, group, mont, sizes=cases.SIZES)


@pytest.mark.parametrize("c,group", cases.PAIRS, ids=cases.PAIR_IDS)
def test_sparse_sums_row_lengths(gpu_ctx, monkeypatch, c, group):
    cases.test_sparse_sums_row_lengths(gpu_ctx, monkeypatch, c, group)


@pytest.mark.parametrize("c,group", cases.PAIRS, ids=cases.PAIR_IDS)
def test_sparse_sums_long_row(gpu_ctx, c, group):
    cases.test_sparse_sums_long_row(gpu_ctx, c, group)


@pytest.mark.parametrize("c,group", cases.PAIRS, ids=cases.PAIR_IDS)
def test_sparse_sums_exceptions(gpu_ctx, monkeypatch, c, group):
    cases.test_sparse_sums_exceptions(gpu_ctx, monkeypatch, c, group)


@pytest.mark.parametrize("c,group", cases.PAIRS, ids=cases.PAIR_IDS)
def test_sparse_sums_chunks(gpu_ctx, monkeypatch, c, group):
    cases.test_sparse_sums_chunks(gpu_ctx, monkeypatch, c, group)


@pytest.mark.parametrize("c,group", cases.PAIRS, ids=cases.PAIR_IDS)
def test_sparse_sums_placement_and_purity(gpu_ctx, c, group):
    cases.test_sparse_sums_placement_and_purity(gpu_ctx, c, group)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_sparse_sums_errors(gpu_ctx, monkeypatch, c):
    cases.test_sparse_sums_errors(gpu_ctx, monkeypatch, c)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_sparse_sums_beyond_one_grid(gpu_ctx, c, n_rows=(1 << 18) + 77, n_general=1000):
    """2^18 + 77 rows of two +-1 terms, 1 000 of them with a general third term, G1: more segments than the 1024 workgroups of 256
    lanes of a row-sum launch hold (the grid-stride loop), and more rows than one pass of anything.  Points [a_j]G from
    ga_batch_scalar_mul on the device; sum_r [z_r] out[r] == [sum z_r (row value)]G by ga_msm over the device-resident output, and the
    rows on either side of the first stride and the last row against the oracle"""
    ctx, wa, n_points = gpu_ctx, affine_words(c.cid, 0), 1 << 12
    rng = np.random.default_rng(0x5BA5 + c.cid)

    def rand_words(n):
        w = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        w[:, 3] = rng.integers(1, c.r >> 192, size=n, dtype=np.uint64)   # below r
        return w, [int.from_bytes(row.tobytes(), "little") for row in w]
    (A, a), (Z, z) = rand_words(n_points), rand_words(n_rows)
    table = cases.coeff_table(c)
    general = [i for i, k in enumerate(table) if cases.magnitude(c, k) > 2]
    cols = rng.integers(0, n_points, size=(n_rows, 3))
    cols[:, 1] = (cols[:, 0] + 1 + cols[:, 1] % (n_points - 1)) % n_points    # two distinct columns per row
    sign = rng.integers(0, 2, size=(n_rows, 2))                               # cid 1 = +1, cid 3 = -1
    stride = 1024 * 256
    special = set(int(x) for x in rng.choice(n_rows, size=n_general, replace=False)) | {stride - 1, stride, n_rows - 1}
    row_start = np.zeros(n_rows + 1, np.uint64)
    length = np.full(n_rows, 2, np.uint64)
    length[sorted(special)] = 3
    row_start[1:] = np.cumsum(length)
    terms = np.zeros((int(row_start[-1]), 2), np.uint32)
    first = row_start[:-1].astype(np.int64)
    for j in (0, 1):
        terms[first + j, 0] = np.where(sign[:, j] == 1, 3, 1)
        terms[first + j, 1] = cols[:, j]
    sp_rows = np.array(sorted(special))
    terms[first[sp_rows] + 2, 0] = np.array(general)[rng.integers(0, len(general), size=sp_rows.size)]
    terms[first[sp_rows] + 2, 1] = cols[sp_rows, 2]

    def value(r):
        return sum(table[int(cid)] * a[int(col)] for cid, col in terms[int(row_start[r]):int(row_start[r + 1])]) % c.r
    sample = [0, stride - 1, stride, stride + 1, n_rows - 1]
    want_pts = fb.expected_points(c, 0, [value(r) for r in sample])
    av = np.array(a, dtype=object)
    assert table[1] == 1 and table[3] == c.r - 1
    tv = np.array([0, 1, 0, -1], dtype=object)                                # cid -> +1 / -1 as signed integers
    total = int((((tv[terms[first, 0]] * av[cols[:, 0]] + tv[terms[first + 1, 0]] * av[cols[:, 1]]) % c.r) * np.array(z, dtype=object)).sum())
    total += sum(table[int(terms[first[r] + 2, 0])] * a[int(cols[r, 2])] * z[r] for r in sp_rows)
    want_sum = oracle.jac_to_affine(c.cid, 0, oracle.generator_mul(c.cid, 0, total % c.r))
    d_pts = ecc.BatchScalarMultiplication(ctx, c.name, 0, fb.gen_arr(c, 0), A, out_device=True)
    d_out = None
    try:
        d_out, redone = ecc.SparsePointSums(ctx, c.name, 0, d_pts, row_start, terms, cases.coeff_arr(c, table), n_points=n_points, out_device=True)
        assert redone == 0
        assert np.array_equal(d_out.to_host((n_rows, wa))[sample], want_pts)
        assert np.array_equal(oracle.jac_to_affine(c.cid, 0, ecc.MultiExp(ctx, c.name, 0, d_out, Z, n=n_rows, montgomery=False)), want_sum)
    finally:
        for b in (d_out, d_pts):
            if b is not None:
                b.free()


@pytest.mark.parametrize("uniform", [1, 0], ids=["uniform", "consecutive"])
@pytest.mark.parametrize("c,group", cases.PAIRS, ids=cases.PAIR_IDS)
def test_lagrange_coeffs_known_tau(gpu_ctx, monkeypatch, c, group, uniform):
    cases.test_lagrange_coeffs_known_tau(gpu_ctx, monkeypatch, c, group, uniform, sizes=cases.LAGRANGE_SIZES + (1024,))


@pytest.mark.parametrize("n", [16, 64, 256])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_lagrange_coeffs_degenerate_g2(gpu_ctx, c, n):
    cases.test_lagrange_coeffs_degenerate_g2(gpu_ctx, c, n)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_lagrange_coeffs_random_g2_points_with_infinities(gpu_ctx, c):
    cases.test_lagrange_coeffs_random_g2_points_with_infinities(gpu_ctx, c)


def test_lagrange_coeffs_g1_is_to_lagrange_g1(gpu_ctx):
    cases.test_lagrange_coeffs_g1_is_to_lagrange_g1(gpu_ctx, n=4096)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_lagrange_coeffs_errors(gpu_ctx, c):
    cases.test_lagrange_coeffs_errors(gpu_ctx, c)


@pytest.mark.parametrize("circuit", list(cases.CIRCUITS))
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_phase2_initialize_replay(gpu_ctx, c, circuit):
    cases.test_phase2_initialize_replay(gpu_ctx, c, circuit)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_phase2_initialize_2_12(gpu_ctx, c, m=1 << 12, n_wires=3000):
    """a random R1CS of 2^12 constraints over 3 000 wires: 64 sampled wires of A, B, B2 and K and 64 sampled points of Z against the
    oracle; then ga_msm over the device-resident A with a random witness == [sum w_i A_i(tau)]G -- no vector leaves the device"""
    ctx = gpu_ctx
    cs = cases.random_r1cs(c, m, n_wires, 0x2C12)
    rng = pyref.Xoshiro(0x2417 + c.cid)
    alpha, beta, tau = (rng.field(c.r - 1) + 1 for _ in range(3))
    n, logs = cases.setup_scalars(c, cs, alpha, beta, tau)
    assert n == m
    out, _ = cases.phase2_initialize(ctx, c, cs, alpha, beta, tau)
    try:
        wires = sorted({0, 1, n_wires - 1} | {rng.next() % n_wires for _ in range(61)})
        zs = sorted({0, 1, n - 2} | {rng.next() % (n - 1) for _ in range(61)})
        for k, g, key, idx, cnt in (("A", 0, "A", wires, n_wires), ("B", 0, "B", wires, n_wires), ("B2", 1, "B", wires, n_wires), ("K", 0, "K", wires, n_wires),
                                    ("Z", 0, "Z", zs, n)):
            got = out[k].to_host((cnt, affine_words(c.cid, g)))
            cases.check(got[idx], fb.expected_points(c, g, [logs[key][i] for i in idx]), k)
            if k == "Z":
                assert not got[n - 1].any()
        w = [rng.field(c.r) for _ in range(n_wires)]
        want = oracle.jac_to_affine(c.cid, 0, oracle.generator_mul(c.cid, 0, sum(x * y for x, y in zip(w, logs["A"])) % c.r))
        assert np.array_equal(oracle.jac_to_affine(c.cid, 0, ecc.MultiExp(ctx, c.name, 0, out["A"], fr_to_arr(c, w), n=n_wires)), want)
    finally:
        for b in out.values():
            b.free()

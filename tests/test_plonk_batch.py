"""ga_plonk_build_z_batch, ga_plonk_quotient_pinned_batch and ga_kzg_open_batch under the functional HIP emulation: `count` proofs of
one circuit per call, and the single calls, which are the one-proof case of the same drivers.  Every batch output is compared byte
for byte with the single call on item j (H after ga_jac_to_affine) -- that checks the splitting into passes, not a second
implementation -- and with an oracle that is no library call: every proof wherever the oracle takes a few seconds at the most (each
case function says where), proof 0 otherwise.  One synthetic
circuit per case (pyref.plonk_synthetic_instance: the fixed polynomials, the permutation and proof 0); the other proofs are
independent random field vectors with random challenges -- the three routines are total functions of their inputs, so a witness need
not satisfy the circuit for the comparison to mean something.  The case functions take the context first;
tests/test_plonk_batch_gpu.py runs them on the device at its sizes."""
import ctypes as C

import numpy as np
import pytest

import oracle
import pyref
from gnark_amd import _lib, ecc, fft, plonk
from gnark_amd.device import jac_words
from helpers import BLS12_381, BN254, arr_to_fr, arr_to_g1_affine, fr_to_arr, jac_to_affine_py

CURVES = [BN254, BLS12_381]
GA_ERR_INVALID = -1
PATTERN = 0xA5A5A5A5A5A5A5A5
_ptr = lambda a: a.ctypes.data_as(C.c_void_p)


def rand_fr(rng, *shape):
    """uniform values below 2^252 (< r on both curves) as (..., 4) fr images"""
    a = rng.integers(0, 1 << 64, size=shape + (4,), dtype=np.uint64)
    a[..., 3] &= np.uint64((1 << 60) - 1)
    return a


def fr_ints(c, a):
    """arr_to_fr for long vectors: the Montgomery factor is inverted once, not per element"""
    rinv = pow(1 << 256, -1, c.r)
    return [int.from_bytes(row.tobytes(), "little") * rinv % c.r for row in np.ascontiguousarray(a, dtype="<u8").reshape(-1, 4)]


def guarded(shape):
    """an output array of `shape` followed by one guard row of the same row shape, all filled with PATTERN"""
    return np.full((shape[0] + 1,) + tuple(shape[1:]), PATTERN, dtype=np.uint64)


def assert_guard(buf, what):
    assert (buf[-1] == PATTERN).all(), what + ": the words after the output changed"


# ---- the circuit and the proofs of a case: computed once per (curve, n, nb_bsb), shared and never written to -------------------------
_circuits = {}


def circuit(c, n, nb_bsb):
    key = (c.name, n, nb_bsb)
    if key not in _circuits:
        lag, qcp, pi2, perm, rng = pyref.plonk_synthetic_instance(c, n, 4100 + n + nb_bsb, nb_bsb)
        beta, gamma, alpha = (rng.field(c.r) for _ in range(3))
        T = dict(perm=np.asarray(perm, dtype=np.int64), beta=beta, gamma=gamma, alpha=alpha, lag_int=lag, qcp_int=qcp, pi2_int=pi2,
                 lag={k: fr_to_arr(c, v) for k, v in lag.items()}, qcp=[fr_to_arr(c, v) for v in qcp], pi2=[fr_to_arr(c, v) for v in pi2],
                 bp_int={k: [rng.field(c.r) for _ in range(3 if k == "Bz" else 2)] for k in ("Bl", "Br", "Bo", "Bz")})
        for a in list(T["lag"].values()) + T["qcp"] + T["pi2"] + [T["perm"]]:
            a.setflags(write=False)
        _circuits[key] = T
    return _circuits[key]


def bitrev_index(n):
    logn = n.bit_length() - 1
    return np.array([int(format(i, "0%db" % logn)[::-1], 2) if logn else 0 for i in range(n)])


def to_canonical(c, a):
    """evaluations on the domain (regular) -> canonical coefficients (regular), by the C oracle's inverse transform"""
    n = a.shape[0]
    return np.ascontiguousarray(oracle.fft(c.cid, a, 1, pyref.DIF, False, nthreads=4)[bitrev_index(n)])


# ---- grand product ---------------------------------------------------------------------------------------------------------------------
def z_inputs(c, n, count):
    """L, R, O (count, n, 4), betas, gammas (count, 4): proof 0 is the synthetic trace; proof 1 has beta = 0; proof 2 has L = R = O = 0"""
    T = circuit(c, n, 0)
    rng = np.random.default_rng([5100 + n, c.cid, count])
    L, R, O = (rand_fr(rng, count, n) for _ in range(3))
    betas, gammas = rand_fr(rng, count), rand_fr(rng, count)
    L[0], R[0], O[0] = T["lag"]["L"], T["lag"]["R"], T["lag"]["O"]
    betas[0], gammas[0] = fr_to_arr(c, [T["beta"]])[0], fr_to_arr(c, [T["gamma"]])[0]
    if count > 1:
        betas[1] = 0
    if count > 2:
        L[2] = R[2] = O[2] = 0
    return T, L, R, O, betas, gammas


def case_build_z(ctx, c, n, count, on_device=False):
    """row j of ga_plonk_build_z_batch == ga_plonk_build_z on item j (one implementation: this tests the splitting into passes);
    EVERY row == pyref.plonk_build_z (linear in n: 0.4 s per row at n = 2^13, the largest size a test uses); the inputs are unchanged
    and the words after the output untouched"""
    lib = ctx.lib
    T, L, R, O, betas, gammas = z_inputs(c, n, count)
    d0 = fft.Domain(ctx, c.name, n)
    try:
        if on_device:
            bufs = [ctx.to_device(v) for v in (L, R, O, T["perm"])]
            out = ctx.to_device(guarded((count, n, 4)))
            try:
                lib.check(lib.ga_plonk_build_z_batch(d0.handle, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, _ptr(betas), _ptr(gammas), count,
                                                     1, out.ptr))
                got = out.to_host((count + 1, n, 4))
                for v, b in zip((L, R, O), bufs):
                    assert np.array_equal(b.to_host(v.shape), v), "an input changed"
            finally:
                out.free()
                for b in bufs:
                    b.free()
        else:
            keep = [x.copy() for x in (L, R, O, betas, gammas)]
            got = guarded((count, n, 4))
            lib.check(lib.ga_plonk_build_z_batch(d0.handle, _ptr(L), _ptr(R), _ptr(O), _ptr(T["perm"]), _ptr(betas), _ptr(gammas), count, 0, _ptr(got)))
            for a, b in zip(keep, (L, R, O, betas, gammas)):
                assert np.array_equal(a, b), "an input changed"
            assert np.array_equal(plonk.BuildRatioCopyConstraintBatch(d0, L, R, O, T["perm"], betas, gammas), got[:count])
        assert_guard(got, "z_out")
        for j in range(count):
            single = plonk.BuildRatioCopyConstraint(d0, L[j], R[j], O[j], T["perm"], betas[j], gammas[j])
            assert np.array_equal(got[j], single), (n, count, j)
        perm = [int(x) for x in T["perm"]]
        for j in range(count):
            want = pyref.plonk_build_z(c, n, fr_ints(c, L[j]), fr_ints(c, R[j]), fr_ints(c, O[j]), perm, fr_ints(c, betas[j])[0], fr_ints(c, gammas[j])[0])
            assert fr_ints(c, got[j]) == want, (n, count, j, "oracle")
    finally:
        d0.close()


@pytest.mark.parametrize("count", [1, 3, 16])
@pytest.mark.parametrize("n", [4, 8, 64, 512])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_build_z_batch(emu_ctx, c, n, count):
    """n = 4 and 8 are smaller than one chunk of the segmented prefix product; proof 1 has beta = 0, proof 2 all-zero wires"""
    case_build_z(emu_ctx, c, n, count)


def test_build_z_batch_on_device(emu_ctx):
    case_build_z(emu_ctx, BN254, 64, 3, on_device=True)


# ---- quotient --------------------------------------------------------------------------------------------------------------------------
def lagrange_names(lagrange, nb_bsb):
    """the per-proof polynomials handed over as evaluations: all of them (True), none (False), or "mixed": R, Z and every Pi2 --
    the driver then reorders its slots (evaluations first) and runs the inverse transforms AND the bit-reversing copy"""
    pi2 = tuple("Pi2%d" % i for i in range(nb_bsb))
    return {True: plonk.PROOF_IDS + pi2, False: (), "mixed": ("R", "Z") + pi2}[lagrange]


def quotient_inputs(c, n, nb_bsb, count, lagrange):
    """the pinned-key inputs and `count` proofs: proof 0 the satisfying trace with Z from the oracle, the others random; with three
    or more proofs the last one repeats proof 1.  lagrange: which per-proof polynomials are evaluations (lagrange_names), the others
    are canonical coefficients"""
    T = circuit(c, n, nb_bsb)
    rng = np.random.default_rng([6100 + n, c.cid, nb_bsb, count, len(lagrange_names(lagrange, nb_bsb))])
    if "Z" not in T:   # the oracle's grand product of the synthetic trace, once per circuit
        T["Z"] = fr_to_arr(c, pyref.plonk_build_z(c, n, T["lag_int"]["L"], T["lag_int"]["R"], T["lag_int"]["O"], [int(x) for x in T["perm"]],
                                                  T["beta"], T["gamma"]))
    Z0 = T["Z"]
    lagr = lagrange_names(lagrange, nb_bsb)
    form = lambda name, a: a if name in lagr else to_canonical(c, a)
    proofs = []
    for j in range(count):
        if j == 0:
            polys = {k: form(k, T["lag"][k]) for k in ("L", "R", "O", "Qk")}
            polys["Z"] = form("Z", Z0)
            pr = dict(polys=polys, pi2=[form("Pi2%d" % i, v) for i, v in enumerate(T["pi2"])], bp={k: fr_to_arr(c, v) for k, v in T["bp_int"].items()},
                      alpha=fr_to_arr(c, [T["alpha"]]), beta=fr_to_arr(c, [T["beta"]]), gamma=fr_to_arr(c, [T["gamma"]]))
        elif j == count - 1 and count >= 3:
            pr = proofs[1]
        else:
            pr = dict(polys={k: rand_fr(rng, n) for k in plonk.PROOF_IDS}, pi2=[rand_fr(rng, n) for _ in range(nb_bsb)],
                      bp={k: rand_fr(rng, 3 if k == "Bz" else 2) for k in ("Bl", "Br", "Bo", "Bz")},
                      alpha=rand_fr(rng, 1), beta=rand_fr(rng, 1), gamma=rand_fr(rng, 1))
        proofs.append(pr)
    return T, proofs


def oracle_quotient(c, n, T, pr, lagrange):
    """h of one proof from the oracle: pyref.plonk_quotient (Python integers) up to n = 64, the C oracle's restatement above"""
    lagr = lagrange_names(lagrange, len(T["qcp"]))
    can = lambda name, a: to_canonical(c, a) if name in lagr else a
    fixed = {k: to_canonical(c, T["lag"][k]) for k in plonk.FIXED_IDS}
    x = dict(fixed, **{k: can(k, pr["polys"][k]) for k in plonk.PROOF_IDS})
    qcp, pi2 = [to_canonical(c, v) for v in T["qcp"]], [can("Pi2%d" % i, v) for i, v in enumerate(pr["pi2"])]
    if n <= 64:
        one = lambda a: arr_to_fr(c, a.reshape(1, 4))[0]
        want = pyref.plonk_quotient(c, n, {k: arr_to_fr(c, v) for k, v in x.items()}, [arr_to_fr(c, v) for v in qcp], [arr_to_fr(c, v) for v in pi2],
                                    {k: arr_to_fr(c, v) for k, v in pr["bp"].items()}, one(pr["alpha"]), one(pr["beta"]), one(pr["gamma"]))
        return fr_to_arr(c, want)
    polys = [x[k] for k in plonk.IDS] + [v for pair in zip(qcp, pi2) for v in pair]
    return oracle.plonk_quotient(c.cid, n, polys, pr["bp"]["Bl"], pr["bp"]["Br"], pr["bp"]["Bo"], pr["bp"]["Bz"], pr["alpha"], pr["beta"],
                                 pr["gamma"], nb_bsb=len(qcp))


def case_quotient(ctx, c, n, nb_bsb, count, lagrange, on_device=False):
    """block j of ga_plonk_quotient_pinned_batch == ga_plonk_quotient_pinned on proof j (one implementation: this tests the splitting
    into passes); every proof up to n = 2^11, proof 0 above (the C oracle takes 1.1 s per proof at 2^13, under 0.1 s up to 2^10: that
    covers every emulation case and the GPU cases of 2^10 and 2^11) == the oracle (pyref.plonk_quotient accepts a witness that does
    not satisfy the circuit: it is the same total function); two proofs with equal inputs give equal blocks; the words after the
    output are untouched"""
    lib = ctx.lib
    T, proofs = quotient_inputs(c, n, nb_bsb, count, lagrange)
    rho = plonk.Rho(n)
    d0, d1 = fft.Domain(ctx, c.name, n), fft.Domain(ctx, c.name, rho * n)
    pk = None
    try:
        pk = plonk.ProvingKey(d0, d1, {k: T["lag"][k] for k in plonk.FIXED_IDS}, T["qcp"],
                              lagrange=plonk.FIXED_IDS + tuple("Qcp%d" % i for i in range(nb_bsb)))
        lagr = lagrange_names(lagrange, nb_bsb)
        if on_device:
            got = quotient_on_device(ctx, pk, proofs, lagr, n, rho)
        else:
            got = pk.ComputeQuotientBatch(proofs, lagrange=lagr)
        assert got.shape[1:] == (rho * n, 4)
        for j, pr in enumerate(proofs):
            single = pk.ComputeQuotient(pr["polys"], pr["pi2"], bp=pr["bp"], alpha=pr["alpha"], beta=pr["beta"], gamma=pr["gamma"], lagrange=lagr)
            assert np.array_equal(got[j], single), (n, nb_bsb, count, j)
        for j in range(count if n <= 1 << 11 else 1):
            assert np.array_equal(got[j], oracle_quotient(c, n, T, proofs[j], lagrange)), (n, nb_bsb, j, "oracle")
        if count >= 3:
            assert np.array_equal(got[1], got[count - 1])
    finally:
        if pk:
            pk.close()
        d0.close()
        d1.close()


def quotient_structs(pk, proofs, lagr, n, keep, device=None):
    """the ga_plonk_quotient_in array of `proofs` (host pointers, or device copies made through device(array))"""
    ins = (_lib.PlonkQuotientIn * len(proofs))()
    for a, pr in zip(ins, proofs):
        a.nb_bsb = pk.nb_bsb
        plonk._fill(a, plonk.PROOF_IDS, pr["polys"], lagr, n, keep)
        pi2 = list(pr["pi2"])
        if device:
            for k in plonk.PROOF_IDS:
                setattr(a, k.lower(), device(pr["polys"][k]))
            pi2 = [device(v) for v in pi2]
            a.flags = 1   # GA_PLONK_ON_DEVICE
        if pi2:
            pa = (C.c_void_p * len(pi2))(*[v if device else v.ctypes.data for v in pi2])
            keep.append(pa)
            a.pi2 = pa
        for k in ("Bl", "Br", "Bo", "Bz"):
            setattr(a, k.lower(), pr["bp"][k].ctypes.data)
        for k in ("alpha", "beta", "gamma"):
            setattr(a, k, pr[k].ctypes.data)
    return ins


def quotient_on_device(ctx, pk, proofs, lagr, n, rho):
    """GA_PLONK_ON_DEVICE: every per-proof polynomial and h_out in device memory; the inputs are unchanged afterwards"""
    lib, keep, bufs = ctx.lib, [], []

    def device(a):
        bufs.append((ctx.to_device(a), a))
        return bufs[-1][0].ptr
    count = len(proofs)
    out = ctx.to_device(guarded((count, rho * n, 4)))
    try:
        ins = quotient_structs(pk, proofs, lagr, n, keep, device)
        lib.check(lib.ga_plonk_quotient_pinned_batch(pk.handle, ins, count, out.ptr))
        got = out.to_host((count + 1, rho * n, 4))
        for b, a in bufs:
            assert np.array_equal(b.to_host(a.shape), a), "an input changed"
    finally:
        out.free()
        for b, _ in bufs:
            b.free()
    assert_guard(got, "h_out")
    return got[:count]


@pytest.mark.parametrize("n,nb_bsb,count,lagrange", [(4, 0, 3, True), (4, 1, 1, False), (8, 1, 3, False), (8, 2, 1, True), (64, 2, 3, True),
                                                     (64, 0, 3, False), (64, 1, 1, False), (8, 1, 3, "mixed"), (64, 2, 3, "mixed")])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_quotient_batch(emu_ctx, c, n, nb_bsb, count, lagrange):
    """n = 4 (rho = 8), 8, 64; nb_bsb 0, 1, 2; one and three proofs; per-proof polynomials as evaluations, as coefficients, and some
    of each (the slots are then reordered)"""
    case_quotient(emu_ctx, c, n, nb_bsb, count, lagrange)


def test_quotient_batch_on_device(emu_ctx):
    case_quotient(emu_ctx, BN254, 8, 1, 3, True, on_device=True)


def test_quotient_batch_host_guard(emu_ctx, c=BN254, n=8, nb_bsb=1, count=3):
    """host pointers through the C ABI: the inputs are unchanged and the words after h_out untouched"""
    ctx, lib = emu_ctx, emu_ctx.lib
    T, proofs = quotient_inputs(c, n, nb_bsb, count, True)
    rho = plonk.Rho(n)
    d0, d1 = fft.Domain(ctx, c.name, n), fft.Domain(ctx, c.name, rho * n)
    pk = plonk.ProvingKey(d0, d1, {k: T["lag"][k] for k in plonk.FIXED_IDS}, T["qcp"], lagrange=plonk.FIXED_IDS + ("Qcp0",))
    try:
        lagr = plonk.PROOF_IDS + ("Pi20",)
        before = [{k: v.copy() for k, v in pr["polys"].items()} for pr in proofs]
        keep, out = [], guarded((count, rho * n, 4))
        lib.check(lib.ga_plonk_quotient_pinned_batch(pk.handle, quotient_structs(pk, proofs, lagr, n, keep), count, _ptr(out)))
        assert_guard(out, "h_out")
        assert np.array_equal(out[:count], pk.ComputeQuotientBatch(proofs, lagrange=lagr))
        for pr, b in zip(proofs, before):
            for k in b:
                assert np.array_equal(pr["polys"][k], b[k]), "an input changed"
    finally:
        pk.close()
        d0.close()
        d1.close()


# ---- opening ---------------------------------------------------------------------------------------------------------------------------
_srs = {}


def srs_of(c, length):
    """`length` G1 bases [k_i]G with known 64-bit k_i (the C oracle multiplies the generator): H of an opening is checked in the exponent"""
    key = (c.name, length)
    if key not in _srs:
        rng = np.random.default_rng([7100 + length, c.cid])
        ks = rng.integers(1, 1 << 63, size=length, dtype=np.uint64)
        pts = oracle.gen_bases(c.cid, 0, ks)
        pts.setflags(write=False)
        _srs[key] = (ks, pts)
    return _srs[key]


def open_inputs(c, length, count):
    """`count` polynomials of `length` coefficients and their points: item 1 is opened at 0, item 2 is a constant polynomial"""
    rng = np.random.default_rng([8100 + length, c.cid, count])
    polys, points = rand_fr(rng, count, length), rand_fr(rng, count)
    if count > 1:
        points[1] = 0
    if count > 2:
        polys[2, 1:] = 0
    return polys, points


def case_open(ctx, c, length, srs_len, count, on_device=False):
    """item j of ga_kzg_open_batch == ga_kzg_open on (polys[j], points[j]): the claimed value byte for byte, H after
    ga_jac_to_affine.  Oracle: every claimed value == Horner in Python integers; every H == [sum_i q_i k_i]G with q from the sequential
    recurrence of pyref.kzg_open's division and the known discrete logs k_i of the SRS; for short polynomials (<= 67 coefficients) H
    == pyref.kzg_open over the SRS points themselves -- item 0 always, every item where length * count <= 200 (its MSM in Python
    integers takes 0.1 s per item at 11 coefficients and 1.2 s at 67: that covers lengths 1, 2 and 11 at every count, and 67 at
    count 1)"""
    lib, mod = ctx.lib, c.r
    ks, pts = srs_of(c, srs_len)
    polys, points = open_inputs(c, length, count)
    table = ecc.PrecomputedBases(ctx, c.name, 0, pts)
    try:
        if on_device:
            bufs = [ctx.to_device(polys[j]) for j in range(count)]
            try:
                arr = (C.c_void_p * count)(*[b.ptr for b in bufs])
                vals, H = guarded((count, 4)), guarded((count, jac_words(c.cid, 0)))
                lib.check(lib.ga_kzg_open_batch(table.handle, arr, length, count, _lib.SCALARS_ON_DEVICE, _ptr(points), _ptr(vals), _ptr(H)))
                for j, b in enumerate(bufs):
                    assert np.array_equal(b.to_host((length, 4)), polys[j]), "an input changed"
            finally:
                for b in bufs:
                    b.free()
        else:
            keep = (polys.copy(), points.copy())
            arr = (C.c_void_p * count)(*[polys[j].ctypes.data for j in range(count)])
            vals, H = guarded((count, 4)), guarded((count, jac_words(c.cid, 0)))
            lib.check(lib.ga_kzg_open_batch(table.handle, arr, length, count, 0, _ptr(points), _ptr(vals), _ptr(H)))
            assert np.array_equal(keep[0], polys) and np.array_equal(keep[1], points), "an input changed"
            v2, H2 = table.KzgOpenBatch(polys, points)
            assert np.array_equal(v2, vals[:count]) and np.array_equal(v2.shape, (count, 4)) and H2.shape == H[:count].shape
        assert_guard(vals, "claimed_values_out")
        assert_guard(H, "h_out")
        zs = arr_to_fr(c, points)
        srs_pts = [arr_to_g1_affine(c, p) for p in pts[:length]] if length <= 67 else None
        for j in range(count):
            sv, sH = table.KzgOpen(polys[j], points[j])
            assert np.array_equal(vals[j], sv), (length, count, j)
            assert jac_to_affine_py(c, 0, H[j]) == jac_to_affine_py(c, 0, sH), (length, count, j)
            p, q, acc = arr_to_fr(c, polys[j]), [0] * max(length - 1, 0), 0
            for k in range(length - 1, 0, -1):
                acc = (p[k] + zs[j] * acc) % mod
                q[k - 1] = acc
            assert arr_to_fr(c, vals[j:j + 1])[0] == (p[0] + zs[j] * acc) % mod, (length, j, "value")
            e = sum(qi * int(ki) for qi, ki in zip(q, ks)) % mod
            assert np.array_equal(oracle.jac_to_affine(c.cid, 0, H[j]), oracle.jac_to_affine(c.cid, 0, oracle.generator_mul(c.cid, 0, e))), (length, j, "H")
            if srs_pts is not None and (j == 0 or length * count <= 200):
                want = pyref.kzg_open(c, srs_pts, p, zs[j])
                assert want[0] == arr_to_fr(c, vals[j:j + 1])[0] and jac_to_affine_py(c, 0, H[j]) == want[1], (length, j, "pyref")
    finally:
        table.free()


@pytest.mark.parametrize("length,srs_len,count", [(1, 4, 3), (2, 4, 3), (67, 70, 1), (67, 70, 17), (257, 300, 3), (515, 520, 3)])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_open_batch(emu_ctx, monkeypatch, c, length, srs_len, count):
    """lengths that are no power of two, an SRS longer than the polynomial, 17 items = 16 + 1; item 1 at the point 0, item 2 constant"""
    monkeypatch.delenv("GA_PLONK_BATCH_MAX", raising=False)
    case_open(emu_ctx, c, length, srs_len, count)


def test_open_above_one_table_block(emu_ctx, monkeypatch):
    """2^12 + 3 coefficients (a blinded polynomial of 2^12 gates): the power tables need a second upper entry, in the batched call and
    in ga_kzg_open -- whose host-built table used to hold floor(n / 2^12) of them, so that coefficient 2^12 and above read past it"""
    monkeypatch.delenv("GA_PLONK_BATCH_MAX", raising=False)
    case_open(emu_ctx, BN254, (1 << 12) + 3, (1 << 12) + 5, 2)


def test_open_batch_on_device(emu_ctx):
    case_open(emu_ctx, BN254, 67, 70, 3, on_device=True)


# ---- chunking --------------------------------------------------------------------------------------------------------------------------
def count_passes(ctx, call):
    """how many device passes each of the three batched calls made inside `call`, from the stage profiler: every pass records its
    ratio-terms launch, its input copies, its division once"""
    ctx.profile(True)
    ctx.profile_reset()
    try:
        call()
        names = [name for name, _ in ctx.profile_read()]
    finally:
        ctx.profile_reset()
        ctx.profile(False)
    return {k: names.count(k) for k in ("plonk_zb_terms", "plonk_qb_h2d", "kzg_b_divide")}


def case_chunks(ctx, monkeypatch, c, n, length, count, batch_max, scan_threads=None):
    """`count` proofs in passes of at most batch_max (None: the default 16): the same comparisons as one pass, and the passes counted.
    scan_threads: GA_PLONK_SCAN_THREADS, so that the segmented scans take chunks wider than 8 at these sizes, and a different width
    for a pass of batch_max proofs than for the remainder pass would take on its own"""
    if batch_max is None:
        monkeypatch.delenv("GA_PLONK_BATCH_MAX", raising=False)
    else:
        monkeypatch.setenv("GA_PLONK_BATCH_MAX", str(batch_max))
    if scan_threads is not None:
        monkeypatch.setenv("GA_PLONK_SCAN_THREADS", str(scan_threads))
    try:
        case_build_z(ctx, c, n, count)
        case_quotient(ctx, c, n, 1, count, True)
        case_open(ctx, c, length, length + 3, count)
        # the knob is honoured: ceil(count / batch_max) passes per call
        T, L, R, O, betas, gammas = z_inputs(c, n, count)
        _, proofs = quotient_inputs(c, n, 1, count, True)
        polys, points = open_inputs(c, length, count)
        rho = plonk.Rho(n)
        d0, d1 = fft.Domain(ctx, c.name, n), fft.Domain(ctx, c.name, rho * n)
        Tq = circuit(c, n, 1)
        pk = plonk.ProvingKey(d0, d1, {k: Tq["lag"][k] for k in plonk.FIXED_IDS}, Tq["qcp"], lagrange=plonk.FIXED_IDS + ("Qcp0",))
        table = ecc.PrecomputedBases(ctx, c.name, 0, srs_of(c, length + 3)[1])
        try:
            def calls():
                plonk.BuildRatioCopyConstraintBatch(d0, L, R, O, T["perm"], betas, gammas)
                pk.ComputeQuotientBatch(proofs, lagrange=lagrange_names(True, 1))
                table.KzgOpenBatch(polys, points)
            want = -(-count // (batch_max or 16))
            assert count_passes(ctx, calls) == {"plonk_zb_terms": want, "plonk_qb_h2d": want, "kzg_b_divide": want}
        finally:
            table.free()
            pk.close()
            d0.close()
            d1.close()
    finally:
        monkeypatch.delenv("GA_PLONK_BATCH_MAX", raising=False)
        monkeypatch.delenv("GA_PLONK_SCAN_THREADS", raising=False)


@pytest.mark.parametrize("count,batch_max", [(5, 2), (17, None)])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_chunks(emu_ctx, monkeypatch, c, count, batch_max):
    """five proofs as 2 + 2 + 1 (GA_PLONK_BATCH_MAX = 2) and seventeen as 16 + 1 (the default)"""
    case_chunks(emu_ctx, monkeypatch, c, 8, 11, count, batch_max)


@pytest.mark.parametrize("scan_threads", [1, 8, 20])
def test_chunks_uneven_passes_and_scan_widths(emu_ctx, monkeypatch, scan_threads, c=BN254):
    """GA_PLONK_BATCH_MAX = 3 on five proofs of 64 gates (3 + 2) with the scans aiming at 1, 8 and 20 threads: the chunk of the prefix
    product is fixed by the first pass (64, 32, 16 elements) where the remainder pass alone would choose 64, 16, 8 -- at 8 and 20
    threads more chunk products (8 and 16) than the first pass reserved (6 and 12), the overrun this case guards; the suffix sums of
    67 coefficients run over wide, middling and 8-element chunks"""
    case_chunks(emu_ctx, monkeypatch, c, 64, 67, 5, 3, scan_threads)


# ---- the single calls: the one-proof case of the same drivers ---------------------------------------------------------------------------
def case_single_build_z(ctx, c, n):
    """ga_plonk_build_z == pyref.plonk_build_z on the synthetic trace and on random wires with beta = 0"""
    T, L, R, O, betas, gammas = z_inputs(c, n, 2)
    d0 = fft.Domain(ctx, c.name, n)
    try:
        for j in range(2):
            got = plonk.BuildRatioCopyConstraint(d0, L[j], R[j], O[j], T["perm"], betas[j], gammas[j])
            want = pyref.plonk_build_z(c, n, arr_to_fr(c, L[j]), arr_to_fr(c, R[j]), arr_to_fr(c, O[j]), [int(x) for x in T["perm"]],
                                       arr_to_fr(c, betas[j:j + 1])[0], arr_to_fr(c, gammas[j:j + 1])[0])
            assert arr_to_fr(c, got) == want, (n, j)
    finally:
        d0.close()


def case_single_open(ctx, c, length, with_open=True):
    """ga_kzg_open and ga_fr_poly_evaluate on a polynomial of `length` coefficients at a random point and at the point 0: the claimed
    value and the evaluation == Horner in Python integers, H == [sum_i q_i k_i]G with q from the sequential recurrence and the known
    discrete logs of the SRS (case_open's check), and up to two coefficients H == pyref.kzg_open over the SRS points.
    with_open=False: the evaluation alone"""
    mod = c.r
    ks, pts = srs_of(c, length + 2)
    polys, points = open_inputs(c, length, 2)   # item 1: the point 0
    zs = arr_to_fr(c, points)
    table = ecc.PrecomputedBases(ctx, c.name, 0, pts) if with_open else None
    try:
        for j in range(2):
            p, q, acc = arr_to_fr(c, polys[j]), [0] * (length - 1), 0
            for k in range(length - 1, 0, -1):
                acc = (p[k] + zs[j] * acc) % mod
                q[k - 1] = acc
            want = (p[0] + zs[j] * acc) % mod
            assert arr_to_fr(c, plonk.Evaluate(ctx, c.name, polys[j], points[j]).reshape(1, 4))[0] == want, (length, j, "evaluate")
            if not with_open:
                continue
            val, H = table.KzgOpen(polys[j], points[j])
            assert arr_to_fr(c, val.reshape(1, 4))[0] == want, (length, j, "value")
            e = sum(qi * int(ki) for qi, ki in zip(q, ks)) % mod
            assert np.array_equal(oracle.jac_to_affine(c.cid, 0, H), oracle.jac_to_affine(c.cid, 0, oracle.generator_mul(c.cid, 0, e))), (length, j, "H")
            if length <= 2:
                ref = pyref.kzg_open(c, [arr_to_g1_affine(c, x) for x in pts[:length]], p, zs[j])
                assert ref[0] == want and jac_to_affine_py(c, 0, H) == ref[1], (length, j, "pyref")
    finally:
        if table:
            table.free()


def case_single_quotient(ctx, c, n, nb_bsb):
    """ga_plonk_quotient_pinned with R, Z and every Pi2 as evaluations and the rest as coefficients == the oracle, on the satisfying
    trace and on a random proof"""
    T, proofs = quotient_inputs(c, n, nb_bsb, 2, "mixed")
    rho = plonk.Rho(n)
    d0, d1 = fft.Domain(ctx, c.name, n), fft.Domain(ctx, c.name, rho * n)
    pk = None
    try:
        pk = plonk.ProvingKey(d0, d1, {k: T["lag"][k] for k in plonk.FIXED_IDS}, T["qcp"],
                              lagrange=plonk.FIXED_IDS + tuple("Qcp%d" % i for i in range(nb_bsb)))
        for j, pr in enumerate(proofs):
            got = pk.ComputeQuotient(pr["polys"], pr["pi2"], bp=pr["bp"], alpha=pr["alpha"], beta=pr["beta"], gamma=pr["gamma"],
                                     lagrange=lagrange_names("mixed", nb_bsb))
            assert np.array_equal(got, oracle_quotient(c, n, T, pr, "mixed")), (n, nb_bsb, j)
    finally:
        if pk:
            pk.close()
        d0.close()
        d1.close()


@pytest.mark.parametrize("scan_threads", [1, 8, 20])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_single_calls_scan_widths(emu_ctx, monkeypatch, c, scan_threads):
    """GA_PLONK_SCAN_THREADS governs the single calls too.  ga_plonk_build_z at n = 2 (the chunk is clamped to n) and n = 512 (two
    chunks of 256 at 1 thread, 64 chunks of 8 at 20); ga_kzg_open and ga_fr_poly_evaluate at 1, 2, 67 and 2^12 + 3 coefficients (no
    quotient coefficient, one, an uneven last chunk, a second upper entry of the power tables), each also at the point 0.  At the
    longest length BLS12-381 runs the evaluation only (the same division over its field): the table MSM of the opening takes seconds
    under the emulation there, and test_open_above_one_table_block opens at that length on BN254 alone as well"""
    monkeypatch.setenv("GA_PLONK_SCAN_THREADS", str(scan_threads))
    for n in (2, 512):
        case_single_build_z(emu_ctx, c, n)
    for length in (1, 2, 67, (1 << 12) + 3):
        case_single_open(emu_ctx, c, length, with_open=c is BN254 or length <= 67)


@pytest.mark.parametrize("n,nb_bsb", [(4, 0), (4, 1), (8, 0), (8, 1)])
def test_single_quotient_mixed_mask(emu_ctx, n, nb_bsb):
    """n = 4 (rho = 8) and n = 8 (rho = 4), without and with a BSB22 gate"""
    case_single_quotient(emu_ctx, BN254, n, nb_bsb)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def case_refusals(ctx, c=BN254, n=8):
    """count = 0 touches nothing; structs that disagree, a null entry of polys, a permutation entry outside [0, 3n), an SRS that is
    too short and null arguments are GA_ERR_INVALID with a message; the next valid call gives the right result"""
    lib = ctx.lib
    T, L, R, O, betas, gammas = z_inputs(c, n, 3)
    _, proofs = quotient_inputs(c, n, 1, 3, True)
    rho = plonk.Rho(n)
    ks, pts = srs_of(c, 8)
    polys, points = open_inputs(c, 8, 3)
    d0, d1 = fft.Domain(ctx, c.name, n), fft.Domain(ctx, c.name, rho * n)
    pk_fixed = circuit(c, n, 1)
    pk = plonk.ProvingKey(d0, d1, {k: pk_fixed["lag"][k] for k in plonk.FIXED_IDS}, pk_fixed["qcp"], lagrange=plonk.FIXED_IDS + ("Qcp0",))
    table = ecc.PrecomputedBases(ctx, c.name, 0, pts)
    lagr = plonk.PROOF_IDS + ("Pi20",)

    def refused(rc, what):
        assert rc == GA_ERR_INVALID, what
        assert lib.ga_last_error(), what

    try:
        parr = (C.c_void_p * 3)(*[polys[j].ctypes.data for j in range(3)])
        perm = T["perm"]
        z_call = lambda count, out, perm=perm, l=L: lib.ga_plonk_build_z_batch(d0.handle, _ptr(l) if l is not None else None, _ptr(R), _ptr(O), _ptr(perm),
                                                                               _ptr(betas), _ptr(gammas), count, 0, _ptr(out))
        keep = []
        q_call = lambda ins, count, out: lib.ga_plonk_quotient_pinned_batch(pk.handle, ins, count, _ptr(out))
        o_call = lambda arr, length, count, vals, H, tab=table: lib.ga_kzg_open_batch(tab.handle, arr, length, count, 0, _ptr(points), _ptr(vals), _ptr(H))
        # count = 0: GA_OK, pre-filled outputs unchanged (null inputs are not even looked at)
        zo, ho, vo, Ho = (np.full(s, PATTERN, dtype=np.uint64) for s in ((3, n, 4), (3, rho * n, 4), (3, 4), (3, jac_words(c.cid, 0))))
        assert z_call(0, zo) == 0 and lib.ga_plonk_build_z_batch(None, None, None, None, None, None, None, 0, 0, None) == 0
        assert q_call(quotient_structs(pk, proofs, lagr, n, keep), 0, ho) == 0 and lib.ga_plonk_quotient_pinned_batch(None, None, 0, None) == 0
        assert o_call(parr, 8, 0, vo, Ho) == 0 and lib.ga_kzg_open_batch(None, None, 0, 0, 0, None, None, None) == 0
        for a in (zo, ho, vo, Ho):
            assert (a == PATTERN).all(), "count = 0 wrote to an output"
        # grand product: a null argument, a permutation entry outside [0, 3n) on the host and on the device
        refused(z_call(3, zo, l=None), "null l")
        for bad in (3 * n, -1):
            p2 = perm.copy()
            p2[5] = bad
            refused(z_call(3, zo, perm=p2), "host permutation")
            bufs = [ctx.to_device(v) for v in (L, R, O, p2)]
            out = ctx.malloc(3 * n * 32)
            try:
                refused(lib.ga_plonk_build_z_batch(d0.handle, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, _ptr(betas), _ptr(gammas), 3, 1, out.ptr),
                        "device permutation")
                assert b"outside" in lib.ga_last_error()
            finally:
                out.free()
                for b in bufs:
                    b.free()
        assert (zo == PATTERN).all()
        assert z_call(3, zo) == 0
        assert np.array_equal(zo[1], plonk.BuildRatioCopyConstraint(d0, L[1], R[1], O[1], perm, betas[1], gammas[1]))
        # quotient: a mismatching lagrange_mask, nb_bsb, flags; a null polynomial; null arguments
        for field, value in (("lagrange_mask", 0), ("nb_bsb", 0), ("flags", 1), ("z", None), ("alpha", None)):
            ins = quotient_structs(pk, proofs, lagr, n, keep)
            setattr(ins[2], field, value)
            refused(q_call(ins, 3, ho), field)
        refused(lib.ga_plonk_quotient_pinned_batch(pk.handle, None, 3, _ptr(ho)), "null ins")
        refused(lib.ga_plonk_quotient_pinned_batch(None, quotient_structs(pk, proofs, lagr, n, keep), 3, _ptr(ho)), "null key")
        assert (ho == PATTERN).all()
        assert q_call(quotient_structs(pk, proofs, lagr, n, keep), 3, ho) == 0
        pr = proofs[1]
        assert np.array_equal(ho[1], pk.ComputeQuotient(pr["polys"], pr["pi2"], bp=pr["bp"], alpha=pr["alpha"], beta=pr["beta"], gamma=pr["gamma"],
                                                        lagrange=lagr))
        # opening: a null entry of polys, an SRS that is too short, an empty polynomial, null arguments
        holed = (C.c_void_p * 3)(polys[0].ctypes.data, None, polys[2].ctypes.data)
        refused(o_call(holed, 8, 3, vo, Ho), "null entry")
        refused(o_call(parr, 0, 3, vo, Ho), "n = 0")
        refused(lib.ga_kzg_open_batch(table.handle, None, 8, 3, 0, _ptr(points), _ptr(vo), _ptr(Ho)), "null polys")
        short = ecc.PrecomputedBases(ctx, c.name, 0, pts[:4])
        try:
            refused(o_call(parr, 8, 3, vo, Ho, tab=short), "short SRS")
            assert b"at least" in lib.ga_last_error()
        finally:
            short.free()
        assert (vo == PATTERN).all() and (Ho == PATTERN).all()
        assert o_call(parr, 8, 3, vo, Ho) == 0
        sv, sH = table.KzgOpen(polys[1], points[1])
        assert np.array_equal(vo[1], sv) and jac_to_affine_py(c, 0, Ho[1]) == jac_to_affine_py(c, 0, sH)
    finally:
        table.free()
        pk.close()
        d0.close()
        d1.close()


def test_refusals(emu_ctx, monkeypatch):
    monkeypatch.delenv("GA_PLONK_BATCH_MAX", raising=False)
    case_refusals(emu_ctx)


def case_exception_barrier(ctx, monkeypatch, c=BN254, n=8):
    """GA_FAULT_THROW set to each of the three entry points: the call returns an error code (no exception crosses the C ABI, the
    context's lock is released); with the knob cleared the same call gives the result it gave before"""
    T, L, R, O, betas, gammas = z_inputs(c, n, 3)
    Tq, proofs = quotient_inputs(c, n, 1, 3, True)
    ks, pts = srs_of(c, 8)
    polys, points = open_inputs(c, 8, 3)
    rho = plonk.Rho(n)
    d0, d1 = fft.Domain(ctx, c.name, n), fft.Domain(ctx, c.name, rho * n)
    pk = plonk.ProvingKey(d0, d1, {k: Tq["lag"][k] for k in plonk.FIXED_IDS}, Tq["qcp"], lagrange=plonk.FIXED_IDS + ("Qcp0",))
    table = ecc.PrecomputedBases(ctx, c.name, 0, pts)
    calls = {
        "ga_plonk_build_z_batch": lambda: plonk.BuildRatioCopyConstraintBatch(d0, L, R, O, T["perm"], betas, gammas),
        "ga_plonk_quotient_pinned_batch": lambda: pk.ComputeQuotientBatch(proofs, lagrange=plonk.PROOF_IDS + ("Pi20",)),
        "ga_kzg_open_batch": lambda: np.concatenate([x.ravel() for x in table.KzgOpenBatch(polys, points)]),
    }
    try:
        for name, call in calls.items():
            before = call()
            monkeypatch.setenv("GA_FAULT_THROW", name)
            with pytest.raises(Exception, match=r"error -3: out of host memory \(std::bad_alloc\) under " + name):
                call()
            monkeypatch.delenv("GA_FAULT_THROW")
            assert np.array_equal(call(), before), name
    finally:
        monkeypatch.delenv("GA_FAULT_THROW", raising=False)
        table.free()
        pk.close()
        d0.close()
        d1.close()


def test_exception_barrier(emu_ctx, monkeypatch):
    case_exception_barrier(emu_ctx, monkeypatch)

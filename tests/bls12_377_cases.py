"""BLS12-377, G1 and Fr: the cases tests/test_bls12_377.py runs on the functional emulation and tests/test_bls12_377_gpu.py on the
device.  Every function takes the context, so the two files differ in sizes only.

The reference is pyref on a pyref.Curve built OUTSIDE the oracle (tools/bls12_377_params.py): pyref's field FFT, PLONK formulas, kzg_open
and G1 group law are generic in the curve.  The C oracle knows two curves and is not involved.

Points with known discrete logs come from ONE scalar multiplication and a chain of additions: P_0 = [K0]G, P_{i+1} = P_i + [DD]G, so
P_i = [K0 + i DD]G and the expected value of an MSM is one multiplication by sum s_i (K0 + i DD) mod r."""
import ctypes as C
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bls12_377_params as Q  # noqa: E402
import pyref  # noqa: E402
from gnark_amd import _lib, ecc, fft, plonk  # noqa: E402
from gnark_amd.device import _ptr  # noqa: E402
from helpers import arr_to_fr, arr_to_g1_affine, fr_to_arr, g1_to_arr, jac_to_affine_py  # noqa: E402

CURVE = Q.curve()
NAME, CID = CURVE.name, CURVE.cid
GRP = pyref.g1_group(CURVE)
R, P = CURVE.r, CURVE.p
K0 = 0x0f1e2d3c4b5a69788796a5b4c3d2e1f00112233445566778899aabbccddeeff1 % R
DD = 0x0123456789abcdef0fedcba987654321123456789abcdef00fedcba987654321 % R

_chain_pts, _chain_logs, _chain_step = [], [], []


def chain(n):
    """(points, dlogs) of the first n chained points; grown on demand, shared by every test of the session"""
    if not _chain_pts:
        _chain_pts.append(GRP.mul(CURVE.g1, K0))
        _chain_logs.append(K0)
        _chain_step.append(GRP.mul(CURVE.g1, DD))
    while len(_chain_pts) < n:
        _chain_pts.append(GRP.add(_chain_pts[-1], _chain_step[0]))
        _chain_logs.append((_chain_logs[-1] + DD) % R)
    return _chain_pts[:n], _chain_logs[:n]


def gmul(k):
    return GRP.mul(CURVE.g1, k % R)


def msm_bases(n):
    """the chain with the operands an MSM has to survive: (0,0), a repeated point, P beside -P (from 7 points up)"""
    pts, logs = (list(v) for v in chain(n))
    if n >= 7:
        pts[1], logs[1] = None, 0
        pts[3], logs[3] = pts[2], logs[2]
        pts[5], logs[5] = GRP.neg(pts[4]), (-logs[4]) % R
    return pts, logs


def digit_scalar(c, plus_one=False):
    """every c-bit digit 2^(c-1): the largest digit that stays positive; plus_one: the lowest digit 2^(c-1) + 1, which turns negative
    and sends a carry into a digit that then turns negative too -- the signed-digit carry chain through every window"""
    s = sum(1 << (c * w + c - 1) for w in range(R.bit_length() // c)) + (1 if plus_one else 0)
    assert s < R
    return s


def msm_scalars(n, seed, widths):
    """random scalars, with 0, 1, r - 1, 2^252, the digit patterns of every window width in `widths` and -- these only make sense in
    canonical form, where the kernel reduces them -- r, r + 1 and 2^256 - 1 in the leading places (as far as n allows)"""
    rng = pyref.Xoshiro(seed)
    s = [rng.field(R) for _ in range(n)]
    special = [0, 1, R - 1, 1 << 252]
    for c in widths:
        special += [digit_scalar(c), digit_scalar(c, True)]
    special += [R, R + 1, (1 << 256) - 1]
    if n < 7:
        return s           # (a single point keeps its random scalar)
    # the specials sit on ordinary chain points (indices 6 ..) where n allows, not on the (0,0) / repeated / negated ones
    at = 6 if n >= 6 + len(special) else 0
    for k, v in enumerate(special[: n - at]):
        s[at + k] = v
    return s


def expected_msm(scalars, logs):
    return gmul(sum(s * k for s, k in zip(scalars, logs)) % R)


def affine(jac):
    return jac_to_affine_py(CURVE, 0, jac)


def jac_sum(lib, parts):
    acc = parts[0]
    for p in parts[1:]:
        acc = ecc.jac_add(NAME, 0, acc, p, lib=lib)
    return acc


# ---- MSM ------------------------------------------------------------------------------------------------------------------------
def case_msm(ctx, n, seed=1):
    """ga_msm in both scalar forms, ga_msm_windows + ga_msm_combine_windows, and a window table: run, run_batch (k = 3), run_windows"""
    lib = ctx.lib
    pts, logs = msm_bases(n)
    Pa = g1_to_arr(CURVE, pts)
    c, nwin = ecc.plan(NAME, 0, n, lib=lib)
    assert nwin == R.bit_length() // c + 1
    T = ecc.PrecomputedBases(ctx, NAME, 0, Pa)
    try:
        tc = T.info()["window_bits"]
        assert T.info()["windows"] == R.bit_length() // tc + 1
        S = msm_scalars(n, seed, {c, tc})
        want = expected_msm(S, logs)
        for mont in (True, False):
            Sa = fr_to_arr(CURVE, [v % R for v in S], True) if mont else np.array([pyref.to_limbs(v, 4) for v in S], dtype=np.uint64)
            got = ecc.MultiExp(ctx, NAME, 0, Pa, Sa, montgomery=mont)
            assert affine(got) == want, ("ga_msm", n, c, mont)
            assert affine(T.MultiExp(Sa, montgomery=mont)) == want, ("ga_msm_table_run", n, tc, mont)
            wins, wc, wn = ecc.MultiExpWindows(ctx, NAME, 0, Pa, Sa, n, 0, -1, montgomery=mont)
            assert (wc, wn) == (c, nwin)
            assert affine(ecc.combine_windows(NAME, 0, wins, wc, lib=lib)) == want, ("ga_msm_windows + combine", n, c, mont)
            tw = T.info()["windows"]
            cut = max(1, tw // 2)
            parts = [T.MultiExpWindows(Sa, 0, cut, montgomery=mont)] + ([T.MultiExpWindows(Sa, cut, tw, montgomery=mont)] if cut < tw else [])
            assert affine(jac_sum(lib, parts)) == want, ("ga_msm_table_run_windows", n, tc, mont)
        vecs = [S, msm_scalars(n, seed + 1, {tc}), msm_scalars(n, seed + 2, {tc})]
        got = T.MultiExpBatch([fr_to_arr(CURVE, [v % R for v in s]) for s in vecs])
        for j, s in enumerate(vecs):
            assert affine(got[j]) == expected_msm(s, logs), ("ga_msm_table_run_batch", n, tc, j)
    finally:
        T.free()
    return c, tc


def case_msm_table_width(ctx, n, table_c, monkeypatch, seed=5):
    """a window table forced to `table_c` bits (GA_TABLE_C): c = 11 and 23 divide the 253 scalar bits, so the top window of
    253 / c + 1 holds the signed-digit carry and nothing else"""
    pts, logs = msm_bases(n)
    Pa = g1_to_arr(CURVE, pts)
    monkeypatch.setenv("GA_TABLE_C", str(table_c))
    T = ecc.PrecomputedBases(ctx, NAME, 0, Pa)
    monkeypatch.delenv("GA_TABLE_C")
    try:
        assert T.info()["window_bits"] == table_c and T.info()["windows"] == R.bit_length() // table_c + 1
        S = msm_scalars(n, seed, {table_c})
        want = expected_msm(S, logs)
        assert affine(T.MultiExp(fr_to_arr(CURVE, [v % R for v in S]))) == want
        assert affine(T.MultiExp(np.array([pyref.to_limbs(v, 4) for v in S], dtype=np.uint64), montgomery=False)) == want
        top = T.info()["windows"] - 1
        parts = [T.MultiExpWindows(fr_to_arr(CURVE, [v % R for v in S]), lo, hi) for lo, hi in ((0, top), (top, top + 1))]
        assert affine(jac_sum(ctx.lib, parts)) == want   # the carry-only window on its own
    finally:
        T.free()


def plan_c11_sizes(lib, limit):
    """every n <= limit for which ga_msm_plan answers c = 11, as (first, last) of each run"""
    runs, start = [], None
    for n in range(1, limit + 1):
        c = ecc.plan(NAME, 0, n, lib=lib)[0]
        if c == 11 and start is None:
            start = n
        if c != 11 and start is not None:
            runs.append((start, n - 1))
            start = None
    if start is not None:
        runs.append((start, limit))
    return runs


def case_group_helpers(lib):
    """ga_generator_mul, ga_jac_scalar_mul, ga_jac_add, ga_jac_to_affine against the python group law"""
    a, b = 0x1234567890abcdef % R, R - 5
    ja, jb = ecc.generator_mul(NAME, 0, a, lib=lib), ecc.generator_mul(NAME, 0, b, lib=lib)
    assert affine(ja) == gmul(a) and affine(jb) == gmul(b)
    assert affine(ecc.jac_add(NAME, 0, ja, jb, lib=lib)) == gmul(a + b)
    assert affine(ecc.jac_scalar_mul(NAME, 0, ja, b, lib=lib)) == gmul(a * b)
    assert arr_to_g1_affine(CURVE, ecc.jac_to_affine(NAME, 0, ja, lib=lib)) == gmul(a)
    assert affine(ecc.generator_mul(NAME, 0, R, lib=lib)) is None


def case_synthetic(ctx, n=96):
    """ga_gen_bases / ga_gen_bases_at (bases with their discrete logs), ga_gen_scalars, ga_fr_dot: the MSM of the synthetic vectors is the
    generator times their dot product"""
    lib = ctx.lib
    wa = 12
    bases, dlogs, sc = ctx.malloc(n * wa * 8), ctx.malloc(n * 32), ctx.malloc(n * 32)
    try:
        lib.check(lib.ga_gen_bases(ctx.handle, CID, 0, 7, n, C.c_void_p(bases.ptr), C.c_void_p(dlogs.ptr)))
        lib.check(lib.ga_gen_scalars(ctx.handle, CID, 9, n, C.c_void_p(sc.ptr)))
        hb, hd, hs = np.zeros((n, wa), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
        for dst, src in ((hb, bases), (hd, dlogs), (hs, sc)):
            lib.check(lib.ga_copy_to_host(ctx.handle, _ptr(dst), C.c_void_p(src.ptr), dst.nbytes))
        logs, scal = arr_to_fr(CURVE, hd, mont=False), arr_to_fr(CURVE, hs)
        assert all(0 < k < (1 << 64) for k in logs) and all(int(x) < R for x in (pyref.from_limbs(r) for r in hs))
        for i in (0, 1, n - 1):
            assert arr_to_g1_affine(CURVE, hb[i]) == gmul(logs[i])
        dot = np.zeros(4, dtype=np.uint64)
        lib.check(lib.ga_fr_dot(ctx.handle, CID, C.c_void_p(sc.ptr), C.c_void_p(dlogs.ptr), n, _ptr(dot)))
        want = sum(a * b for a, b in zip(scal, logs)) % R
        assert pyref.from_limbs(dot) == want
        assert affine(ecc.MultiExp(ctx, NAME, 0, bases, sc, n=n)) == gmul(want)
        # element `first + i` of the same sequence
        part = ctx.malloc(8 * wa * 8)
        lib.check(lib.ga_gen_bases_at(ctx.handle, CID, 0, 7, n - 8, 8, C.c_void_p(part.ptr), None))
        hp = np.zeros((8, wa), dtype=np.uint64)
        lib.check(lib.ga_copy_to_host(ctx.handle, _ptr(hp), C.c_void_p(part.ptr), hp.nbytes))
        part.free()
        assert np.array_equal(hp, hb[n - 8:])
    finally:
        for b in (bases, dlogs, sc):
            b.free()


# ---- NTT ------------------------------------------------------------------------------------------------------------------------
def case_fft(ctx, n, seed=3):
    """ga_fft: DIF and DIT, forward and inverse, on the coset and off it, against pyref.fft"""
    rng = pyref.Xoshiro(seed + n)
    a = [rng.field(R) for _ in range(n)]
    A = fr_to_arr(CURVE, a)
    d = fft.Domain(ctx, NAME, n)
    try:
        for dec in (pyref.DIF, pyref.DIT):
            for coset in (False, True):
                assert arr_to_fr(CURVE, d.FFT(A, dec, coset)) == pyref.fft(CURVE, a, dec, on_coset=coset), ("FFT", n, dec, coset)
                assert arr_to_fr(CURVE, d.FFTInverse(A, dec, coset)) == pyref.fft(CURVE, a, dec, on_coset=coset, inverse=True), ("iFFT", n, dec, coset)
    finally:
        d.close()


def case_fft_batch(ctx, n=1 << 10, count=3):
    rng = pyref.Xoshiro(17)
    vs = [[rng.field(R) for _ in range(n)] for _ in range(count)]
    A = np.stack([fr_to_arr(CURVE, v) for v in vs])
    d = fft.Domain(ctx, NAME, n)
    try:
        got = d.FFTBatch(A, pyref.DIF, on_coset=True)
        inv = d.FFTInverseBatch(A, pyref.DIT)
        for j, v in enumerate(vs):
            assert arr_to_fr(CURVE, got[j]) == pyref.fft(CURVE, v, pyref.DIF, on_coset=True), ("ga_fft_batch", j)
            assert arr_to_fr(CURVE, inv[j]) == pyref.fft(CURVE, v, pyref.DIT, inverse=True), ("ga_fft_batch inverse", j)
    finally:
        d.close()


def case_compute_h(ctx, m=(1 << 10) - 5):
    rng = pyref.Xoshiro(23)
    a, b = [rng.field(R) for _ in range(m)], [rng.field(R) for _ in range(m)]
    c = [x * y % R for x, y in zip(a, b)]
    d = fft.Domain(ctx, NAME, m)
    try:
        want = pyref.compute_h(CURVE, a, b, c, d.Cardinality)
        assert arr_to_fr(CURVE, d.compute_h(fr_to_arr(CURVE, a), fr_to_arr(CURVE, b), fr_to_arr(CURVE, c))) == want
        two = d.compute_h_batch(*(np.stack([fr_to_arr(CURVE, v)] * 2) for v in (a, b, c)))
        assert arr_to_fr(CURVE, two[0]) == want and arr_to_fr(CURVE, two[1]) == want
    finally:
        d.close()


# ---- PLONK ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def plonk_instance(n, nb_bsb):
    """a satisfying synthetic trace (Lagrange form), its grand product and quotient from pyref: computed once per shape"""
    lag, qcp, pi2, perm, prng = pyref.plonk_synthetic_instance(CURVE, n, 5 + n + nb_bsb, nb_bsb)
    beta, gamma, alpha = (prng.field(R) for _ in range(3))
    lag["Z"] = pyref.plonk_build_z(CURVE, n, lag["L"], lag["R"], lag["O"], perm, beta, gamma)
    w0, ninv = CURVE.fr_root_of_unity(n), pow(n, -1, R)
    can = lambda v: [x * ninv % R for x in pyref._ntt_natural(v, pow(w0, -1, R), R)]
    bp = {k: [prng.field(R) for _ in range(3 if k == "Bz" else 2)] for k in ("Bl", "Br", "Bo", "Bz")}
    want = pyref.plonk_quotient(CURVE, n, {k: can(v) for k, v in lag.items()}, [can(q) for q in qcp], [can(p) for p in pi2], bp, alpha, beta, gamma)
    return dict(lag=lag, qcp=qcp, pi2=pi2, perm=perm, beta=beta, gamma=gamma, alpha=alpha, bp=bp, h=want)


def _quotient_args(I):
    f = lambda v: fr_to_arr(CURVE, v)
    return dict(bp={k: f(v) for k, v in I["bp"].items()}, alpha=f([I["alpha"]]), beta=f([I["beta"]]), gamma=f([I["gamma"]]))


def case_plonk(ctx, n, nb_bsb):
    """ga_plonk_build_z, ga_plonk_quotient and ga_plonk_pk_create + ga_plonk_quotient_pinned against pyref"""
    I = plonk_instance(n, nb_bsb)
    lag, f = I["lag"], lambda v: fr_to_arr(CURVE, v)
    d0, d1 = fft.Domain(ctx, NAME, n), fft.Domain(ctx, NAME, plonk.Rho(n) * n)
    try:
        Z = plonk.BuildRatioCopyConstraint(d0, f(lag["L"]), f(lag["R"]), f(lag["O"]), I["perm"], f([I["beta"]]), f([I["gamma"]]))
        assert arr_to_fr(CURVE, Z) == lag["Z"], ("ga_plonk_build_z", n)
        names = tuple(plonk.IDS) + tuple(x for i in range(nb_bsb) for x in ("Qcp%d" % i, "Pi2%d" % i))
        hq = plonk.ComputeQuotient(d0, d1, {k: f(lag[k]) for k in plonk.IDS}, [f(q) for q in I["qcp"]], [f(p) for p in I["pi2"]],
                                   lagrange=names, **_quotient_args(I))
        assert arr_to_fr(CURVE, hq) == I["h"], ("ga_plonk_quotient", n, nb_bsb)
        pk = plonk.ProvingKey(d0, d1, {k: f(lag[k]) for k in plonk.FIXED_IDS}, [f(q) for q in I["qcp"]],
                              lagrange=tuple(plonk.FIXED_IDS) + tuple("Qcp%d" % i for i in range(nb_bsb)))
        try:
            hp = pk.ComputeQuotient({k: f(lag[k]) for k in plonk.PROOF_IDS}, [f(p) for p in I["pi2"]],
                                    lagrange=tuple(plonk.PROOF_IDS) + tuple("Pi2%d" % i for i in range(nb_bsb)), **_quotient_args(I))
            assert arr_to_fr(CURVE, hp) == I["h"], ("ga_plonk_quotient_pinned", n, nb_bsb)
        finally:
            pk.close()
    finally:
        d0.close()
        d1.close()


def srs(n):
    """[tau^i]G for i < n with a known tau: the dlogs, and the points by one python multiplication each (computed once)"""
    return _srs(n)


TAU = 0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe % R


@functools.lru_cache(maxsize=4)
def _srs(n):
    logs = [pow(TAU, i, R) for i in range(n)]
    return [gmul(k) for k in logs], logs


def case_kzg_open(ctx, n=1 << 8):
    """ga_kzg_open against pyref.kzg_open: the claimed value, and the commitment to the quotient over [tau^i]G"""
    pts, _ = srs(n)
    rng = pyref.Xoshiro(29)
    poly, z = [rng.field(R) for _ in range(n)], rng.field(R)
    want_v, want_h = pyref.kzg_open(CURVE, pts, poly, z)
    T = ecc.PrecomputedBases(ctx, NAME, 0, g1_to_arr(CURVE, pts))
    try:
        val, h = T.KzgOpen(fr_to_arr(CURVE, poly), fr_to_arr(CURVE, [z]))
        assert arr_to_fr(CURVE, val)[0] == want_v and affine(h) == want_h
    finally:
        T.free()


def case_plonk_batches(ctx, monkeypatch, n=1 << 8, count=3):
    """the three _batch calls with `count` proofs in passes of at most two (GA_PLONK_BATCH_MAX = 2) and short scan chunks
    (GA_PLONK_SCAN_THREADS = 4): every proof equals its single call, which case_plonk / case_kzg_open hold against pyref"""
    f = lambda v: fr_to_arr(CURVE, v)
    I = plonk_instance(n, 1)
    lag = I["lag"]
    rng = pyref.Xoshiro(31)
    proofs = []
    for _ in range(count):   # one circuit, `count` witnesses' worth of challenges and blinding: the per-proof operands
        bp = {k: f([rng.field(R) for _ in range(3 if k == "Bz" else 2)]) for k in ("Bl", "Br", "Bo", "Bz")}
        proofs.append(dict(bp=bp, alpha=f([rng.field(R)]), beta=f([rng.field(R)]), gamma=f([rng.field(R)])))
    d0, d1 = fft.Domain(ctx, NAME, n), fft.Domain(ctx, NAME, plonk.Rho(n) * n)
    pts, _ = srs(n)
    T = ecc.PrecomputedBases(ctx, NAME, 0, g1_to_arr(CURVE, pts), batched=True)
    pk = plonk.ProvingKey(d0, d1, {k: f(lag[k]) for k in plonk.FIXED_IDS}, [f(I["qcp"][0])], lagrange=tuple(plonk.FIXED_IDS) + ("Qcp0",))
    try:
        L, Rr, O = f(lag["L"]), f(lag["R"]), f(lag["O"])
        single_z = [plonk.BuildRatioCopyConstraint(d0, L, Rr, O, I["perm"], p["beta"], p["gamma"]) for p in proofs]
        names = tuple(plonk.PROOF_IDS) + ("Pi20",)
        polys = [dict({k: f(lag[k]) for k in ("L", "R", "O", "Qk")}, Z=z) for z in single_z]
        single_h = [pk.ComputeQuotient(polys[j], [f(I["pi2"][0])], lagrange=names, **proofs[j]) for j in range(count)]
        kp = [f([rng.field(R) for _ in range(n)]) for _ in range(count)]
        kz = f([rng.field(R) for _ in range(count)])
        single_k = [T.KzgOpen(kp[j], kz[j]) for j in range(count)]
        monkeypatch.setenv("GA_PLONK_BATCH_MAX", "2")
        monkeypatch.setenv("GA_PLONK_SCAN_THREADS", "4")
        Zb = plonk.BuildRatioCopyConstraintBatch(d0, np.stack([L] * count), np.stack([Rr] * count), np.stack([O] * count), I["perm"],
                                                 np.concatenate([p["beta"] for p in proofs]), np.concatenate([p["gamma"] for p in proofs]))
        Hb = pk.ComputeQuotientBatch([dict(polys=polys[j], pi2=[f(I["pi2"][0])], **proofs[j]) for j in range(count)], lagrange=names)
        vals, hs = T.KzgOpenBatch(kp, kz)
        for j in range(count):
            assert np.array_equal(Zb[j], single_z[j]), ("ga_plonk_build_z_batch", j)
            assert np.array_equal(Hb[j], single_h[j]), ("ga_plonk_quotient_pinned_batch", j)
            assert np.array_equal(vals[j], single_k[j][0]) and affine(hs[j]) == affine(single_k[j][1]), ("ga_kzg_open_batch", j)
    finally:
        pk.close()
        T.free()
        d0.close()
        d1.close()


def case_fr_vectors(ctx, n=300):
    """ga_fr_batch_invert (a zero entry stays zero), ga_fr_linear_combination, ga_fr_poly_evaluate, ga_fr_vec_mul, ga_hash_to_field"""
    from gnark_amd import groth16
    rng = pyref.Xoshiro(37)
    v = [rng.field(R) for _ in range(n)]
    v[0], v[n // 2], v[n - 1] = 0, 0, 1
    got = arr_to_fr(CURVE, plonk.BatchInvert(ctx, NAME, fr_to_arr(CURVE, v)))
    assert got == [pow(x, -1, R) if x else 0 for x in v]
    vecs = [[rng.field(R) for _ in range(n)] for _ in range(5)]
    sc = [rng.field(R) for _ in range(5)]
    lc = plonk.LinearCombination(ctx, NAME, fr_to_arr(CURVE, sc), [fr_to_arr(CURVE, x) for x in vecs])
    assert arr_to_fr(CURVE, lc) == [sum(s * x[i] for s, x in zip(sc, vecs)) % R for i in range(n)]
    for z in (0, 1, R - 1, rng.field(R)):
        assert arr_to_fr(CURVE, plonk.Evaluate(ctx, NAME, fr_to_arr(CURVE, v), fr_to_arr(CURVE, [z])))[0] == pyref._poly_eval(v, z, R)
    a, b = fr_to_arr(CURVE, vecs[0]), fr_to_arr(CURVE, vecs[1])
    out = np.zeros_like(a)
    ctx.lib.check(ctx.lib.ga_fr_vec_mul(ctx.handle, CID, _ptr(a), _ptr(b), n, _ptr(out), 0))
    assert arr_to_fr(CURVE, out) == [x * y % R for x, y in zip(vecs[0], vecs[1])]
    for msg, dst, cnt in ((b"", b"d", 1), (b"bls12-377 transcript", b"G16-BSB22", 3)):
        assert arr_to_fr(CURVE, groth16.HashToField(NAME, msg, dst, cnt, lib=ctx.lib)) == pyref.fr_hash(CURVE, msg, dst, cnt)


# ---- SRS ------------------------------------------------------------------------------------------------------------------------
def case_batch_scalar_mul(ctx, n=1 << 8):
    """ga_batch_scalar_mul on the generator: scalar i is K0 + i DD, so result i is chain point i (the reference is the python group law's
    additions); the scalars an SRS never has -- 0, 1, r - 1, r + 1, 2^256 - 1 -- by a python multiplication each.  Both scalar forms."""
    pts, logs = chain(n)
    special = [0, 1, R - 1, R + 1, (1 << 256) - 1]
    sc = list(logs)
    sc[:len(special)] = special
    want = [gmul(s) for s in special] + list(pts[len(special):])
    base = g1_to_arr(CURVE, [CURVE.g1])
    can = np.array([pyref.to_limbs(s, 4) for s in sc], dtype=np.uint64)
    got = ecc.BatchScalarMultiplication(ctx, NAME, 0, base, can)
    assert [arr_to_g1_affine(CURVE, row) for row in got] == want, "ga_batch_scalar_mul, canonical scalars"
    got = ecc.BatchScalarMultiplication(ctx, NAME, 0, base, fr_to_arr(CURVE, [s % R for s in sc]), montgomery=True)
    assert [arr_to_g1_affine(CURVE, row) for row in got] == want, "ga_batch_scalar_mul, Montgomery scalars"
    c, nw = ecc.batch_scalar_mul_plan(NAME, n, lib=ctx.lib)
    assert c >= 1 and nw * c >= R.bit_length()


@functools.lru_cache(maxsize=4)
def lagrange_srs(n):
    """[l_i(tau)]G, i < n: l(tau) is the inverse DFT of the powers of tau"""
    _, logs = srs(n)
    li = pyref.fft(CURVE, bitrev_in(logs), pyref.DIT, inverse=True)
    return [gmul(k) for k in li]


def bitrev_in(v):
    return pyref.bitrev_permute(list(v))   # DIT takes bit-reversed input and gives natural output


def case_to_lagrange(ctx, n):
    pts, _ = srs(n)
    got = ecc.ToLagrangeG1(ctx, NAME, g1_to_arr(CURVE, pts))
    assert [arr_to_g1_affine(CURVE, row) for row in got] == lagrange_srs(n), ("ga_kzg_to_lagrange_g1", n)


# ---- ga_check_points --------------------------------------------------------------------------------------------------------------
def check_points_input():
    """64 points: chain points, (0,0), an image with a coordinate not below p, (x, y + 1), and three points on the curve outside the
    subgroup that need no square root: (-1, 0) of order 2, (0, 1) of order 3, [k]G + (-1, 0)"""
    pts, _ = chain(64)
    rows = g1_to_arr(CURVE, pts)
    want = np.zeros(64, dtype=np.uint8)
    rows[9] = 0                                                     # (0,0): accepted, as gnark-crypto does
    x_img = pyref.from_limbs(rows[20][:6]) + P                      # the Montgomery image of x, plus p: still 384 bits, not reduced
    assert x_img < 1 << 384
    rows[20][:6] = pyref.to_limbs(x_img, 6)
    want[20] = ecc.POINT_OFF_CURVE
    rows[33] = g1_to_arr(CURVE, [(pts[33][0], (pts[33][1] + 1) % P)])[0]
    want[33] = ecc.POINT_OFF_CURVE
    two, three = (P - 1, 0), (0, 1)
    mixed = GRP.add(pts[50], two)
    for Pt in (two, three, mixed):
        assert GRP.on_curve(Pt) and GRP.mul(Pt, R) is not None
    assert GRP.add(two, two) is None and GRP.mul(three, 3) is None
    for i, Pt in ((41, two), (42, three), (50, mixed)):
        rows[i] = g1_to_arr(CURVE, [Pt])[0]
        want[i] = ecc.POINT_NOT_IN_SUBGROUP
    return rows, want


def case_check_points(ctx, monkeypatch):
    rows, want = check_points_input()
    for naive in (None, "1"):
        if naive:
            monkeypatch.setenv("GA_CHECK_NAIVE", naive)
        else:
            monkeypatch.delenv("GA_CHECK_NAIVE", raising=False)
        status, off, outside, first, redone = ecc.CheckPoints(ctx, NAME, 0, rows)
        assert list(status) == list(want), ("status", naive)
        assert (off, outside, first) == (2, 3, 20), ("counters", naive, off, outside, first)
        assert redone <= 3, ("honest points never take the exact kernel", naive, redone)
        cs, coff, cout, cfirst, _ = ecc.CheckPoints(ctx, NAME, 0, rows, curve_only=True)
        assert (coff, cout, cfirst) == (2, 0, 20) and [int(s) for s in cs] == [1 if w == ecc.POINT_OFF_CURVE else 0 for w in want]
    monkeypatch.delenv("GA_CHECK_NAIVE", raising=False)
    ok = g1_to_arr(CURVE, chain(64)[0])
    assert ecc.CheckPoints(ctx, NAME, 0, ok)[1:] == (0, 0, ecc.NONE_BAD, 0)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _refused(lib, rc):
    msg = lib.ga_last_error().decode()
    assert rc != _lib.GA_OK, "the call was accepted"
    assert "bls12-377" in msg and "unknown curve" not in msg, msg
    return msg


def case_refusals(ctx):
    """every out-of-scope call with curve 2, and in-scope calls with (2, GA_G2), answer an error that names bls12-377; the same call
    with BN254 operands then succeeds in the same context"""
    from gnark_amd import g16_setup, groth16
    lib, h = ctx.lib, ctx.handle
    bn = pyref.BN254

    def operands(c):
        g1 = g1_to_arr(c, [c.g1] * 4)
        g2w = 4 * c.fp_limbs
        g2 = np.zeros((4, g2w), dtype=np.uint64)
        if c is bn:
            from helpers import g2_to_arr
            g2 = g2_to_arr(c, [c.g2] * 4)
        fr = fr_to_arr(c, [1, 2, 3, 4])
        return c.cid, g1, g2, fr

    row_start = np.array([0, 1, 2], dtype=np.uint64)
    terms = np.array([[0, 0], [1, 1]], dtype=np.uint32)
    out2, ok = (C.c_uint64 * 2)(), np.zeros(1, dtype=np.uint8)

    def calls(c):
        cid, g1, g2, fr = operands(c)
        name = c.name
        builder = C.c_void_p()

        def builder_create():
            rc = lib.ga_g16_builder_create(h, cid, 4, 3, 0, 1, C.byref(builder))
            if rc == _lib.GA_OK:
                lib.ga_g16_builder_destroy(builder)
            return rc

        def wrap(fn):
            def run():
                try:
                    fn()
                except _lib.GnarkAmdError:
                    return 1
                return _lib.GA_OK
            return run
        fold_out = np.zeros(2 * c.fp_limbs, dtype=np.uint64)
        return {
            "ga_pairing_check": lambda: lib.ga_pairing_check(h, cid, _ptr(g1), _ptr(g2), 1, None, 1, 0, _ptr(ok), None, out2),
            "ga_g16_builder_create": builder_create,
            "ga_g16_fold_pok": lambda: lib.ga_g16_fold_pok(cid, _ptr(g1), 2, _ptr(fr), _ptr(fold_out)),
            "ga_g16_proof_unmarshal": wrap(lambda: groth16.ParseProof(name, pyref_proof_bytes(), lib=lib)),
            "ga_scale_points": wrap(lambda: ecc.ScalePoints(ctx, name, 0, g1, fr, montgomery=True)),
            "ga_scale_points G2": wrap(lambda: ecc.ScalePoints(ctx, name, 1, g2, fr, montgomery=True)),
            "ga_sparse_point_sums": wrap(lambda: ecc.SparsePointSums(ctx, name, 0, g1, row_start, terms, fr, montgomery=True)),
            "ga_lagrange_coeffs": wrap(lambda: ecc.LagrangeCoeffs(ctx, name, 0, g1)),
            "ga_fr_lagrange_at": wrap(lambda: g16_setup.LagrangeAt(ctx, name, 4, fr[1:2].copy(), montgomery=True)),
            "ga_fr_sparse_matvec": wrap(lambda: g16_setup.SparseMatVec(ctx, name, fr, row_start, terms, fr, montgomery=True)),
            "ga_fr_compact_nonzero": wrap(lambda: g16_setup.CompactNonZero(ctx, name, fr)),
            "ga_fr_powers": wrap(lambda: g16_setup.Powers(ctx, name, fr[0:1].copy(), fr[1:2].copy(), 4, montgomery=True)),
            # calls that are in scope for G1: G2 is refused
            "ga_msm G2": wrap(lambda: ecc.MultiExp(ctx, name, 1, g2, fr)),
            "ga_msm_windows G2": wrap(lambda: ecc.MultiExpWindows(ctx, name, 1, g2, fr, 4, 0, -1)),
            "ga_msm_plan G2": wrap(lambda: ecc.plan(name, 1, 4, lib=lib)),
            "ga_msm_table_create G2": wrap(lambda: ecc.PrecomputedBases(ctx, name, 1, g2).free()),
            "ga_batch_scalar_mul G2": wrap(lambda: ecc.BatchScalarMultiplication(ctx, name, 1, g2[0], fr, montgomery=True)),
            "ga_check_points G2": wrap(lambda: ecc.CheckPoints(ctx, name, 1, g2)),
            "ga_generator_mul G2": wrap(lambda: ecc.generator_mul(name, 1, 5, lib=lib)),
            "ga_jac_add G2": wrap(lambda: ecc.jac_add(name, 1, np.zeros(6 * c.fp_limbs, dtype=np.uint64), np.zeros(6 * c.fp_limbs, dtype=np.uint64), lib=lib)),
            "ga_jac_to_affine G2": wrap(lambda: ecc.jac_to_affine(name, 1, np.zeros(6 * c.fp_limbs, dtype=np.uint64), lib=lib)),
            "ga_jac_scalar_mul G2": wrap(lambda: ecc.jac_scalar_mul(name, 1, np.zeros(6 * c.fp_limbs, dtype=np.uint64), 3, lib=lib)),
            "ga_msm_combine_windows G2": wrap(lambda: ecc.combine_windows(name, 1, np.zeros((2, 6 * c.fp_limbs), dtype=np.uint64), 4, lib=lib)),
            "ga_gen_bases G2": lambda: _gen_bases_g2(ctx, cid, c.fp_limbs),
        }

    refused, accepted = calls(CURVE), calls(bn)
    for name in refused:
        _refused(lib, refused[name]())
        assert accepted[name]() == _lib.GA_OK, (name, "on BN254", lib.ga_last_error().decode())
    # a key description that names curve 2 is refused before anything is read from it or staged
    key, pk = _lib.G16Key(), C.c_void_p()
    key.curve, key.domain_cardinality = CID, 4
    _refused(lib, lib.ga_g16_pk_create(h, C.byref(key), C.byref(pk)))
    assert not pk.value
    # curve 7 stays an unknown curve
    assert lib.ga_msm_plan(7, 0, 4, C.byref(C.c_int()), C.byref(C.c_int())) != _lib.GA_OK and "unknown curve" in lib.ga_last_error().decode()


def _gen_bases_g2(ctx, cid, fp):
    buf = ctx.malloc(2 * 4 * fp * 8)
    try:
        return ctx.lib.ga_gen_bases(ctx.handle, cid, 1, 3, 2, C.c_void_p(buf.ptr), None)
    finally:
        buf.free()


@functools.lru_cache(maxsize=1)
def pyref_proof_bytes():
    """a BN254 Groth16 proof's bytes (three generator multiples): what ga_g16_proof_unmarshal parses for BN254 and refuses to look at
    for curve 2"""
    c = pyref.BN254
    return pyref.proof_bytes(c, pyref.g1_group(c).mul(c.g1, 5), pyref.g2_group(c).mul(c.g2, 7), pyref.g1_group(c).mul(c.g1, 11))

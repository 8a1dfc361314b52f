"""ga_fft_batch, ga_compute_h_batch and ga_g16_prove_batch under the functional HIP emulation: `count` transforms / quotient
vectors / proofs of one size in one call, element for element against the C oracle and pyref (a library call is never the
reference).  Every function takes the context first; tests/test_prove_batch_gpu.py runs the same cases on the device at its sizes."""
import ctypes as C
import threading

import numpy as np
import pytest

import oracle
import pyref
from gnark_amd import fft, groth16
from gnark_amd.device import affine_words
from helpers import BLS12_381, BN254, arr_to_fr, fr_to_arr, pts_to_arr
from test_emu_kernels import FFT_MODES, FORCED_PLAN_CASES, FORCED_PLAN_KNOB_CASES, NTT_KNOBS

CURVES = [BN254, BLS12_381]
GA_ERR_INVALID, GA_ERR_STATE = -1, -4
_ptr = lambda a: a.ctypes.data_as(C.c_void_p)


# ---- batched transforms ----------------------------------------------------------------------------------------------------------
_vec_cache = {}


def _vectors(c, logn, count):
    """`count` different uniform vectors of 2^logn residues and the C oracle's eight transforms of each: computed once per
    (curve, size), shared by the cases and never written to"""
    key = (c.name, logn)
    have = _vec_cache.get(key, ([], []))
    rng = np.random.default_rng([7700 + logn, c.cid, len(have[0])])
    while len(have[0]) < count:
        a = fr_to_arr(c, [int.from_bytes(rng.bytes(40), "little") % c.r for _ in range(1 << logn)])
        want = {m: oracle.fft(c.cid, a, m[0], m[1], m[2], nthreads=4) for m in FFT_MODES}
        for x in [a] + list(want.values()):
            x.setflags(write=False)
        have[0].append(a)
        have[1].append(want)
        rng = np.random.default_rng([7700 + logn, c.cid, len(have[0])])
    _vec_cache[key] = have
    return have[0][:count], have[1][:count]


def _run(d, inv):
    return d.FFTInverseBatch if inv else d.FFTBatch


@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("logn", [0, 1, 3, 9, 10])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_fft_batch_all_modes(emu_ctx, c, logn, count):
    """all eight modes on `count` different vectors in one call: a tile smaller than the workgroup's 1024 slots (2^3, 2^9), exactly
    one tile (2^10), the identity sizes 2^0 and 2^1; each output vector is the oracle's transform of its own input"""
    vecs, want = _vectors(c, logn, count)
    d = fft.Domain(emu_ctx, c.name, 1 << logn)
    try:
        for m in FFT_MODES:
            inv, dec, coset = m
            got = _run(d, inv)(np.stack(vecs), dec, coset)
            assert got.shape == (count, 1 << logn, 4)
            for j in range(count):
                assert np.array_equal(got[j], want[j][m]), (logn, m, j)
    finally:
        d.close()


@pytest.mark.parametrize("logn", [3, 10])
def test_fft_batch_containment(emu_ctx, logn, c=BN254, count=3):
    """the device buffer holds count + 1 vectors and the call is told `count`: the last one, a sentinel pattern, is unchanged; and
    vector j's result does not depend on its neighbours: the same vector alone gives the same words"""
    ctx = emu_ctx
    n = 1 << logn
    vecs, want = _vectors(c, logn, count)
    sentinel = np.full((n, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    d = fft.Domain(ctx, c.name, n)
    try:
        for m in ((0, pyref.DIF, True), (1, pyref.DIT, False), (0, pyref.DIT, True)):
            inv, dec, coset = m
            buf = ctx.to_device(np.concatenate([np.stack(vecs), sentinel[None]]))
            try:
                _run(d, inv)(buf, dec, coset, count=count)
                got = buf.to_host((count + 1, n, 4))
            finally:
                buf.free()
            assert np.array_equal(got[count], sentinel), m
            for j in range(count):
                assert np.array_equal(got[j], want[j][m]), (m, j)
                alone = _run(d, inv)(vecs[j][None], dec, coset)
                assert np.array_equal(alone[0], got[j]), (m, j)
    finally:
        d.close()


def _forced_plan_batch(ctx, monkeypatch, c, plan, knobs, count=2):
    logn = sum(int(k) for k in plan.split(","))
    vecs, want = _vectors(c, logn, count)
    for k, v in NTT_KNOBS[knobs].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("GA_NTT_PLAN", plan)   # read by ntt_plan when the domain is created
    try:
        d = fft.Domain(ctx, c.name, 1 << logn)
    finally:
        monkeypatch.delenv("GA_NTT_PLAN")
    try:
        for m in FFT_MODES:
            inv, dec, coset = m
            got = _run(d, inv)(np.stack(vecs), dec, coset)
            for j in range(count):
                assert np.array_equal(got[j], want[j][m]), (plan, knobs, m, j)
    finally:
        d.close()


@pytest.mark.parametrize("c,plan", FORCED_PLAN_CASES, ids=lambda v: getattr(v, "name", v))
def test_fft_batch_forced_plans(emu_ctx, monkeypatch, c, plan):
    """every pass shape GA_NTT_PLAN can produce (the plan list of test_emu_fft_forced_plans) with a batch of two: the slot mapping
    must not depend on the batch index"""
    _forced_plan_batch(emu_ctx, monkeypatch, c, plan, "default")


@pytest.mark.parametrize("plan,knobs", FORCED_PLAN_KNOB_CASES)
def test_fft_batch_forced_plans_knobs(emu_ctx, monkeypatch, plan, knobs):
    _forced_plan_batch(emu_ctx, monkeypatch, BN254, plan, knobs)


_h_cache = {}


def _h_triples(c, logn, short, count):
    """`count` triples (A, B, C = A o B, but the last one with a random C) of n - short constraints and the oracle's computeH of each"""
    key = (c.name, logn, short, count)
    if key not in _h_cache:
        n = 1 << logn
        rng = np.random.default_rng([8800 + logn, c.cid, short])
        uni = lambda: fr_to_arr(c, [int.from_bytes(rng.bytes(40), "little") % c.r for _ in range(n - short)])
        out = []
        for j in range(count):
            A, B = uni(), uni()
            Cc = uni() if j == count - 1 else oracle.fr_mul(c.cid, A, B)
            out.append((A, B, Cc, oracle.compute_h(c.cid, A, B, Cc, n, nthreads=4)))
        _h_cache[key] = out
    return _h_cache[key]


@pytest.mark.parametrize("short", [5, 0], ids=["n-5", "n"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_compute_h_batch(emu_ctx, c, short, logn=6, count=3):
    """ga_compute_h_batch on three triples with n_constraints = n - 5 (the padding kernel) and = n, from host pointers and from
    device pointers: every h is the oracle's computeH of its own triple"""
    ctx, lib = emu_ctx, emu_ctx.lib
    n = 1 << logn
    T = _h_triples(c, logn, short, count)
    A, B, Cc = (np.stack([t[k] for t in T]) for k in range(3))
    d = fft.Domain(ctx, c.name, n)
    try:
        got = d.compute_h_batch(A, B, Cc)
        for j in range(count):
            assert np.array_equal(got[j], T[j][3]), ("host", j)
        bufs = [ctx.to_device(v) for v in (A, B, Cc)]
        out = ctx.malloc(count * n * 32)
        try:
            lib.check(lib.ga_compute_h_batch(d.handle, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, count, n - short, out.ptr, 1))
            got = out.to_host((count, n, 4))
            for v, b in zip((A, B, Cc), bufs):   # the inputs are left as they were
                assert np.array_equal(b.to_host(v.shape), v)
        finally:
            out.free()
            for b in bufs:
                b.free()
        for j in range(count):
            assert np.array_equal(got[j], T[j][3]), ("device", j)
    finally:
        d.close()


def test_fft_batch_errors(emu_ctx, c=BN254, logn=4):
    """null data and n_constraints > n are GA_ERR_INVALID, count = 0 is GA_OK and touches nothing; the same valid call succeeds
    afterwards"""
    ctx, lib = emu_ctx, emu_ctx.lib
    n = 1 << logn
    vecs, want = _vectors(c, logn, 2)
    m = (0, pyref.DIF, False)
    d = fft.Domain(ctx, c.name, n)
    try:
        a = np.stack(vecs)
        assert lib.ga_fft_batch(d.handle, None, 2, 0, pyref.DIF, 0, 0) == GA_ERR_INVALID
        assert lib.ga_fft_batch(d.handle, _ptr(a), 2, 7, pyref.DIF, 0, 0) == GA_ERR_INVALID
        keep = a.copy()
        assert lib.ga_fft_batch(d.handle, _ptr(a), 0, 0, pyref.DIF, 0, 0) == 0 and np.array_equal(a, keep)
        assert lib.ga_fft_batch(d.handle, None, 0, 0, pyref.DIF, 0, 0) == 0
        got = d.FFTBatch(a, pyref.DIF)
        assert np.array_equal(got[0], want[0][m]) and np.array_equal(got[1], want[1][m])
        T = _h_triples(c, logn, 0, 2)
        A, B, Cc = (np.stack([t[k] for t in T]) for k in range(3))
        out = np.zeros((2, n, 4), np.uint64)
        assert lib.ga_compute_h_batch(d.handle, _ptr(A), _ptr(B), _ptr(Cc), 2, n + 1, _ptr(out), 0) == GA_ERR_INVALID
        assert b"n_constraints" in lib.ga_last_error()
        assert lib.ga_compute_h_batch(d.handle, _ptr(A), None, _ptr(Cc), 2, n, _ptr(out), 0) == GA_ERR_INVALID
        assert lib.ga_compute_h_batch(d.handle, None, None, None, 0, n, None, 0) == 0
        got = d.compute_h_batch(A, B, Cc)
        assert np.array_equal(got[0], T[0][3]) and np.array_equal(got[1], T[1][3])
    finally:
        d.close()


# ---- batch proofs ----------------------------------------------------------------------------------------------------------------
# The synthetic key of test_emu_groth16_synthetic_vs_c_oracle / test_emu_groth16_mixed_vector_layouts, restated: bases [k_i]G from
# ga_gen_bases (seeds 1 .. 7), nbWires = n, three public wires, InfinityA on wires {1, 5, nw - 1}; "dense": InfinityB on {0, 7}, so
# that with tables A, B, K and G2.B are wire-indexed; "mixed": InfinityB on every second wire, so that G1.B and G2.B get compact tables
# (G2.B walking G1.B's digits) beside wire-indexed A and K; "plain": the dense key pinned without tables.
KEY_KINDS = {"dense": 1, "mixed": 1, "plain": -1}
NB_PUBLIC = 3
_key_cache, _sol_cache, _want_cache = {}, {}, {}


def _gen(ctx, c, group, count, seed):
    buf = ctx.malloc(count * affine_words(c.cid, group) * 8)
    ctx.lib.check(ctx.lib.ga_gen_bases(ctx.handle, c.cid, group, seed, count, buf.ptr, None))
    h = buf.to_host((count, affine_words(c.cid, group)))
    buf.free()
    return h


def _scal(ctx, c, count, seed):
    buf = ctx.malloc(count * 32)
    ctx.lib.check(ctx.lib.ga_gen_scalars(ctx.handle, c.cid, seed, count, buf.ptr))
    h = buf.to_host((count, 4))
    buf.free()
    return h


def synthetic_key(ctx, c, logn, kind):
    """the key's fields as host arrays (what groth16.ProvingKey takes; with n added, what oracle.groth16_prove takes)"""
    mask = "mixed" if kind == "mixed" else "dense"
    ck = (c.name, logn, mask)
    if ck not in _key_cache:
        n = nw = 1 << logn
        infA, infB = np.zeros(nw, np.uint8), np.zeros(nw, np.uint8)
        infA[[1, 5, nw - 1]] = 1
        if mask == "mixed":
            infB[1::2] = 1
        else:
            infB[[0, 7]] = 1
        nb = nw - int(infB.sum())
        m1, m2 = _gen(ctx, c, 0, 3, 1), _gen(ctx, c, 1, 2, 2)
        _key_cache[ck] = dict(alpha1=m1[0:1], beta1=m1[1:2], delta1=m1[2:3], A=_gen(ctx, c, 0, nw - 3, 3), B=_gen(ctx, c, 0, nb, 4),
                              Z=_gen(ctx, c, 0, n - 1, 5), K=_gen(ctx, c, 0, nw - NB_PUBLIC, 6), beta2=m2[0:1], delta2=m2[1:2],
                              B2=_gen(ctx, c, 1, nb, 7), infinityA=infA, infinityB=infB)
    return _key_cache[ck]


def solutions(ctx, c, logn, count):
    """`count` solutions with distinct W, A, B, C = A o B, r and s; entry 1 is the all-zero solution"""
    ck = (c.name, logn)
    have = _sol_cache.setdefault(ck, [])
    n = 1 << logn
    m = n - 9
    while len(have) < count:
        j = len(have)
        if j == 1:
            W, A, B = (np.zeros((k, 4), np.uint64) for k in (n, m, m))
        else:
            W, A, B = _scal(ctx, c, n, 100 + 10 * j), _scal(ctx, c, m, 101 + 10 * j), _scal(ctx, c, m, 102 + 10 * j)
        rs = _scal(ctx, c, 2, 103 + 10 * j)
        have.append((groth16.Solution(W, A, B, oracle.fr_mul(c.cid, A, B)), rs[0], rs[1]))
    return have[:count]


def oracle_proofs(ctx, c, logn, kind, count):
    """the C oracle's proof points of the first `count` solutions under the key, computed once each"""
    mask = "mixed" if kind == "mixed" else "dense"
    key = dict(synthetic_key(ctx, c, logn, kind), n=1 << logn)
    out = []
    for j, (sol, r, s) in enumerate(solutions(ctx, c, logn, count)):
        ck = (c.name, logn, mask, j)
        if ck not in _want_cache:
            _want_cache[ck] = oracle.groth16_prove(c.cid, key, sol.W, sol.A, sol.B, sol.C, NB_PUBLIC, r, s, nthreads=8)
        out.append(_want_cache[ck])
    return out


def pin(ctx, c, logn, kind, **kw):
    return groth16.ProvingKey(ctx, c.name, domain_cardinality=1 << logn, precompute=KEY_KINDS[kind], **synthetic_key(ctx, c, logn, kind), **kw)


def prove_batch(pk, sols):
    return groth16.ProveBatch(pk, [x[0] for x in sols], NB_PUBLIC, np.stack([x[1] for x in sols]), np.stack([x[2] for x in sols]))


def assert_proofs(proofs, want, what):
    assert len(proofs) == len(want), what
    for j, (p, w) in enumerate(zip(proofs, want)):
        assert np.array_equal(p.Ar, w[0]) and np.array_equal(p.Bs, w[1]) and np.array_equal(p.Krs, w[2]), (what, j)


def check_layout(pk, kind):
    """the key takes the paths the case is about (so that a case cannot silently test another one)"""
    lay = groth16.ShardLayout(pk)
    if kind == "plain":
        assert not any(lay["tables"].values()), lay
    else:
        assert lay["tables"] == dict(A=True, B=True, Z=True, K=True, B2=True), lay
        wire = dict(A=True, B=True, K=True, B2=True) if kind == "dense" else dict(A=True, B=False, K=True, B2=False)
        assert lay["wire_indexed"] == wire, lay


@pytest.mark.parametrize("kind", list(KEY_KINDS))
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_prove_batch_layouts(emu_ctx, monkeypatch, c, kind, logn=6, count=3):
    """three solutions (the second all zeros) in one batch under the three keys that cover every layout path -- wire-indexed tables
    over the one sort of the three witnesses, compact tables with G2.B on G1.B's digits, plain vectors looped: every proof's three
    points are the C oracle's for its entry"""
    ctx = emu_ctx
    for k in ("GA_G16_SHARE_MIN_PCT", "GA_G16_TABLE_BUDGET_PCT", "GA_G16_BATCH_MAX"):
        monkeypatch.delenv(k, raising=False)
    want = oracle_proofs(ctx, c, logn, kind, count)
    pk = pin(ctx, c, logn, kind)
    try:
        check_layout(pk, kind)
        assert_proofs(prove_batch(pk, solutions(ctx, c, logn, count)), want, kind)
    finally:
        pk.FreeGPUResources()


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_prove_batch_chunks(emu_ctx, monkeypatch, c, logn=6, count=5):
    """GA_G16_BATCH_MAX = 2 walks five solutions as chunks of 2 + 2 + 1, GA_G16_BATCH_MAX = 1 one by one: the oracle's points, and the
    same proof bytes either way"""
    ctx = emu_ctx
    want = oracle_proofs(ctx, c, logn, "dense", count)
    sols = solutions(ctx, c, logn, count)
    pk = pin(ctx, c, logn, "dense")
    try:
        monkeypatch.setenv("GA_G16_BATCH_MAX", "2")
        got = prove_batch(pk, sols)
        assert_proofs(got, want, "chunks of 2")
        monkeypatch.setenv("GA_G16_BATCH_MAX", "1")
        one = prove_batch(pk, sols)
        assert [p.WriteTo() for p in one] == [p.WriteTo() for p in got]
    finally:
        monkeypatch.delenv("GA_G16_BATCH_MAX", raising=False)
        pk.FreeGPUResources()


def _pinned_circuit_key(ctx, c, pk, precompute, **kw):
    return groth16.ProvingKey(
        ctx, c.name, domain_cardinality=pk.n, alpha1=pts_to_arr(c, 0, [pk.alpha1]), beta1=pts_to_arr(c, 0, [pk.beta1]),
        delta1=pts_to_arr(c, 0, [pk.delta1]), A=pts_to_arr(c, 0, pk.A), B=pts_to_arr(c, 0, pk.B), Z=pts_to_arr(c, 0, pk.Z),
        K=pts_to_arr(c, 0, pk.K), beta2=pts_to_arr(c, 1, [pk.beta2]), delta2=pts_to_arr(c, 1, [pk.delta2]), B2=pts_to_arr(c, 1, pk.B2),
        infinityA=pk.infinityA, infinityB=pk.infinityB, precompute=precompute, **kw)


def _solution_of(c, cs, w):
    A, B, Cc = pyref.r1cs_solve(c, cs, w)
    return groth16.Solution(W=fr_to_arr(c, w), A=fr_to_arr(c, A), B=fr_to_arr(c, B), C=fr_to_arr(c, Cc))


@pytest.mark.parametrize("precompute", [1, -1], ids=["tables", "no-tables"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_prove_batch_cubic(emu_ctx, c, precompute):
    """examples/cubic with two different inputs in one batch: Proof.WriteTo() bytes equal pyref's"""
    rng = pyref.Xoshiro(2025)
    cs = pyref.cubic_r1cs()
    pk, _, _ = pyref.groth16_setup(c, cs, [rng.field(c.r) for _ in range(5)])
    ws = [pyref.cubic_witness(3), pyref.cubic_witness(5)]
    rs, ss = [rng.field(c.r) for _ in ws], [rng.field(c.r) for _ in ws]
    dpk = _pinned_circuit_key(emu_ctx, c, pk, precompute)
    try:
        proofs = groth16.ProveBatch(dpk, [_solution_of(c, cs, w) for w in ws], cs.nb_public, fr_to_arr(c, rs), fr_to_arr(c, ss))
    finally:
        dpk.FreeGPUResources()
    for w, r, s, proof in zip(ws, rs, ss, proofs):
        assert proof.WriteTo() == pyref.proof_bytes(c, *pyref.groth16_prove(pk, cs, w, r, s)), w


@pytest.mark.parametrize("precompute", [1, -1], ids=["tables", "no-tables"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_prove_batch_bsb22(emu_ctx, c, precompute):
    """the two-commitment circuit of pyref with two different inputs: the commitments are made per solution with ga_g16_commit (the
    solver's hint), then both are proved in one call; K's scalars go through the remove list for every solution of the batch.  The
    bytes, commitments and folded proof of knowledge included, equal pyref's."""
    ctx, lib = emu_ctx, emu_ctx.lib
    rng = pyref.Xoshiro(4243)
    cs = pyref.commit_r1cs()
    pk, _, _ = pyref.groth16_setup(c, cs, [rng.field(c.r) for _ in range(5 + len(cs.commitments) + 1)])
    removed = sorted({j for cm in cs.commitments for j in cm.private_committed} | {cm.commitment_index for cm in cs.commitments})
    dpk = _pinned_circuit_key(ctx, c, pk, precompute, k_remove=removed,
                              commitment_keys=[(pts_to_arr(c, 0, b), pts_to_arr(c, 0, e)) for b, e in pk.commitment_keys])
    fbytes = (c.r.bit_length() - 1) // 8 + 1
    inputs = [(3, 11), (5, 7)]
    ws, coms, poks = [], [], []
    try:
        for x, y in inputs:
            com, pok = {}, {}

            def hint(i, w):   # the bsb22 hint override (prove.go:72-100) with the device doing the MSMs
                cm = cs.commitments[i]
                com[i], pok[i] = dpk.Commit(i, fr_to_arr(c, [w[j] for j in cm.private_committed]))
                msg = groth16.MarshalG1(c.name, com[i], lib=lib) + b"".join(int(w[j]).to_bytes(fbytes, "big") for j in cm.public_and_commitment_committed)
                return arr_to_fr(c, groth16.HashToField(c.name, msg, groth16.COMMITMENT_DST, 1, lib=lib))[0]

            ws.append(pyref.commit_solve(c, cs, x, y, hint))
            coms.append(com)
            poks.append(pok)
        rs, ss = [rng.field(c.r) for _ in ws], [rng.field(c.r) for _ in ws]
        proofs = groth16.ProveBatch(dpk, [_solution_of(c, cs, w) for w in ws], cs.nb_public, fr_to_arr(c, rs), fr_to_arr(c, ss))
    finally:
        dpk.FreeGPUResources()
    ncm = len(cs.commitments)
    for w, r, s, proof, com, pok in zip(ws, rs, ss, proofs, coms, poks):
        ser = b"".join(int(w[cm.commitment_index]).to_bytes(32, "big") for cm in cs.commitments)
        challenge = groth16.HashToField(c.name, ser, groth16.FOLD_DST, 1, lib=lib)
        proof.Commitments = np.stack([com[i] for i in range(ncm)])
        proof.CommitmentPok = groth16.FoldPok(c.name, np.stack([pok[i] for i in range(ncm)]), challenge, lib=lib)
        ar, bs, krs, ocoms, opok = pyref.groth16_prove_bsb22(pk, cs, w, r, s)
        assert proof.WriteTo() == pyref.proof_bytes(c, ar, bs, krs, ocoms, opok), w


def _raw_batch(lib, pk, sols, n_constraints, nb_public=NB_PUBLIC, null_w=None):
    """ga_g16_prove_batch through ctypes, with room for a bad argument: returns (code, proof images)"""
    count = len(sols)
    arrs = [[np.ascontiguousarray(getattr(x[0], f), dtype=np.uint64) for x in sols] for f in "WABC"]
    ptrs = [(C.c_void_p * count)(*[a.ctypes.data for a in col]) for col in arrs]
    if null_w is not None:
        ptrs[0][null_w] = None
    rs, ss = np.stack([x[1] for x in sols]), np.stack([x[2] for x in sols])
    out = np.zeros((count, 8 * (4 if pk.curve == 0 else 6)), np.uint64)
    rc = lib.ga_g16_prove_batch(pk.handle, count, ptrs[0], ptrs[1], ptrs[2], ptrs[3], n_constraints, nb_public, _ptr(rs), _ptr(ss), _ptr(out))
    return rc, out


def test_prove_batch_refusals(emu_ctx, c=BN254, logn=6, count=3):
    """a share of a sharded key is GA_ERR_STATE; a null w[1] (named in the message), n_constraints = n + 1 and an nb_public the key
    contradicts are GA_ERR_INVALID; count = 0 is GA_OK; after each refusal the valid batch gives the bytes it gave before"""
    ctx, lib = emu_ctx, emu_ctx.lib
    n = 1 << logn
    sols = solutions(ctx, c, logn, count)
    nc = sols[0][0].A.shape[0]
    pk = pin(ctx, c, logn, "dense")
    shard = pin(ctx, c, logn, "dense", shard=(0, 2))
    try:
        rc, before = _raw_batch(lib, pk, sols, nc)
        assert rc == 0
        assert_proofs([groth16.Proof(c.cid, o[:8], o[8:24], o[24:]) for o in before], oracle_proofs(ctx, c, logn, "dense", count), "raw call")

        def still_fine():
            rc, again = _raw_batch(lib, pk, sols, nc)
            assert rc == 0 and np.array_equal(again, before)
        rc, _ = _raw_batch(lib, shard, sols, nc)
        assert rc == GA_ERR_STATE and b"one share of a sharded key" in lib.ga_last_error()
        still_fine()
        rc, _ = _raw_batch(lib, pk, sols, nc, null_w=1)
        assert rc == GA_ERR_INVALID and b"w[1]" in lib.ga_last_error()
        still_fine()
        rc, _ = _raw_batch(lib, pk, sols, n + 1)
        assert rc == GA_ERR_INVALID and b"exceed the domain cardinality" in lib.ga_last_error()
        still_fine()
        rc, _ = _raw_batch(lib, pk, sols, nc, nb_public=NB_PUBLIC + 1)
        assert rc == GA_ERR_INVALID and b"inconsistent sizes" in lib.ga_last_error()
        still_fine()
        assert lib.ga_g16_prove_batch(pk.handle, 0, None, None, None, None, nc, NB_PUBLIC, None, None, None) == 0
        assert lib.ga_g16_prove_batch(None, 2, None, None, None, None, nc, NB_PUBLIC, None, None, None) == GA_ERR_INVALID
        still_fine()
    finally:
        shard.FreeGPUResources()
        pk.FreeGPUResources()


def test_prove_batch_exception_barrier(emu_ctx, monkeypatch, c=BN254, logn=6):
    """GA_FAULT_THROW set to each of the three new entry points: the call returns an error code (the exception does not cross the C
    ABI, locks and key use are released); with the knob cleared the same call gives the result it gave before"""
    ctx = emu_ctx
    n = 1 << logn
    vecs, _ = _vectors(c, logn, 2)
    T = _h_triples(c, logn, 5, 2)
    A, B, Cc = (np.stack([t[k] for t in T]) for k in range(3))
    sols = solutions(ctx, c, logn, 3)
    d = fft.Domain(ctx, c.name, n)
    pk = pin(ctx, c, logn, "dense")
    calls = {
        "ga_fft_batch": lambda: d.FFTBatch(np.stack(vecs), fft.DIF, True),
        "ga_compute_h_batch": lambda: d.compute_h_batch(A, B, Cc),
        "ga_g16_prove_batch": lambda: np.stack([p.raw() for p in prove_batch(pk, sols)]),
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
        pk.FreeGPUResources()
        d.close()


def test_prove_batch_beside_single_proof(emu_ctx, c=BN254, logn=6, rounds=2):
    """supported concurrent use: one thread runs ProveBatch on four solutions while a second runs Prove on the same key with a fifth,
    for two rounds; all five proofs are the oracle's every time"""
    ctx = emu_ctx
    want = oracle_proofs(ctx, c, logn, "dense", 5)
    sols = solutions(ctx, c, logn, 5)
    pk = pin(ctx, c, logn, "dense")
    got, errs = {}, []

    def batch():
        try:
            for k in range(rounds):
                got["batch", k] = prove_batch(pk, sols[:4])
        except Exception as e:   # (reported by the main thread)
            errs.append(e)

    def single():
        try:
            for k in range(rounds):
                got["single", k] = groth16.Prove(pk, sols[4][0], NB_PUBLIC, sols[4][1], sols[4][2])
        except Exception as e:
            errs.append(e)
    try:
        threads = [threading.Thread(target=batch), threading.Thread(target=single)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    finally:
        pk.FreeGPUResources()
    assert not errs, errs
    for k in range(rounds):
        assert_proofs(got["batch", k], want[:4], ("batch", k))
        assert_proofs([got["single", k]], want[4:], ("single", k))

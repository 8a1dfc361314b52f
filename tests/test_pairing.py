"""Pairing products (ga_pairing_check, gnark_amd/csrc/pairing.hip.h) and the Groth16 verifier built on them (gnark_amd/g16_verify.py)
on the functional emulation.  Every case is a function of a context; tests/test_pairing_gpu.py runs the same cases on the device.
Expected values come from the model (pyref.pairing_check, pyref.groth16_verify, pyref.Fp12Ops) or from construction (a group closed
by the pair (-[sum a_i b_i]G1, G2)), never from the library."""
import base64
import ctypes as C
import json
import os

import numpy as np
import pytest

import pyref
import test_check_points as cp
import test_fixed_base as fb
import test_scale_points as sp
from gnark_amd import ecc, g16_verify, groth16
from gnark_amd.device import affine_words
from helpers import BLS12_381, BN254, arr_to_g1_affine, arr_to_g2_affine, pts_to_arr

CURVES = [BN254, BLS12_381]
NONE_BAD = (1 << 64) - 1
EDGE_SIZES = (1, 2, 63, 64, 65, 257)


class knobs:
    """GA_PAIRING_CHUNK for the calls inside the block (read once per entry point)"""

    def __init__(self, monkeypatch, chunk=None):
        self.mp, self.env = monkeypatch, {"GA_PAIRING_CHUNK": chunk}

    def __enter__(self):
        for k, v in self.env.items():
            if v is None:
                self.mp.delenv(k, raising=False)
            else:
                self.mp.setenv(k, str(v))

    def __exit__(self, *a):
        for k in self.env:
            self.mp.delenv(k, raising=False)


def logs_a(c, n):
    return sp.logs(c, n)


def logs_b(c, n):
    return sp.rand_scalars(c, n, seed=7)


def pairs(c, a, b):
    """([a_i]G1, [b_i]G2) as two arrays"""
    return fb.expected_points(c, 0, [x % c.r for x in a]).copy(), fb.expected_points(c, 1, [x % c.r for x in b]).copy()


def closing(c, a, b):
    """the logs of the pair that closes prod e([a_i]G1, [b_i]G2) to 1: (-sum a_i b_i, 1)"""
    return (-sum(x * y for x, y in zip(a, b))) % c.r, 1


def model_pairs(c, P, Q):
    return [(arr_to_g1_affine(c, p), arr_to_g2_affine(c, q)) for p, q in zip(P, Q)]


def model_ok(c, P, Q, gs):
    mp = model_pairs(c, P, Q)
    return np.array([1 if pyref.pairing_check(c, mp[gs[g]:gs[g + 1]]) else 0 for g in range(len(gs) - 1)], np.uint8)


def summary(want):
    bad = np.nonzero(want == 0)[0]
    return int(bad.size), int(bad[0]) if bad.size else NONE_BAD


def gt_to_model(c, row):
    """12 fp.Element images in E12 order -> pyref's coefficients of w^0..w^11: the Fp2 at C_i.B_j goes through embed_fp2(., 2j + i)"""
    F12 = pyref.Fp12Ops(c)
    n = c.fp_limbs
    v = [pyref.from_mont_limbs([int(x) for x in row[k * n:(k + 1) * n]], c.p) for k in range(12)]
    out = [0] * 12
    for i in range(2):
        for j in range(3):
            k = 2 * (3 * i + j)
            e = F12.embed_fp2((v[k], v[k + 1]), 2 * j + i)
            out = [(s + t) % c.p for s, t in zip(out, e)]
    return out


# ---- 1. against the oracle ----------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_case(c):
    """16 random pairs cut into {0..3}, {4}, {} and {5..15}; the same with pair 15 replaced by the pair that closes the last group;
    the model's verdicts for both"""
    if c.cid not in _ORACLE:
        a, b = logs_a(c, 16), logs_b(c, 16)
        gs = [0, 4, 5, 5, 16]
        P, Q = pairs(c, a, b)
        ca, cb = closing(c, a[5:15], b[5:15])
        P2, Q2 = pairs(c, a[:15] + [ca], b[:15] + [cb])
        _ORACLE[c.cid] = (gs, (P, Q, model_ok(c, P, Q, gs)), (P2, Q2, model_ok(c, P2, Q2, gs)))
    return _ORACLE[c.cid]


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_pairing_against_oracle(emu_ctx, c):
    """ok and out2 equal pyref.pairing_check group by group; the empty group is 1; closing the last group turns it to 1"""
    gs, open_case, closed_case = oracle_case(c)
    assert list(open_case[2]) == [0, 0, 1, 0] and list(closed_case[2]) == [0, 0, 1, 1]
    for P, Q, want in (open_case, closed_case):
        ok, bad, first = ecc.PairingCheck(emu_ctx, c.name, P, Q, gs)
        assert np.array_equal(ok, want) and (bad, first) == summary(want)


# ---- 2. by construction, at the edges ------------------------------------------------------------------------------------------------------
_EDGES = {}


def edge_case(c):
    """groups of 1, 2, 63, 64, 65 and 257 pairs, each closed to 1 by its last pair; (P, Q, group_start, a): a the logs of P"""
    if c.cid not in _EDGES:
        n = sum(EDGE_SIZES)
        a, b = list(logs_a(c, n)), list(logs_b(c, n))
        gs = [0]
        for s in EDGE_SIZES:
            lo, hi = gs[-1], gs[-1] + s
            a[hi - 1], b[hi - 1] = closing(c, a[lo:hi - 1], b[lo:hi - 1])
            gs.append(hi)
        P, Q = pairs(c, a, b)
        _EDGES[c.cid] = (P, Q, gs, a)
    return _EDGES[c.cid]


def perturbed(c, P, a, idx):
    out = P.copy()
    for i in idx:
        out[i] = fb.expected_points(c, 0, [(a[i] + 1) % c.r])[0]
    return out


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_pairing_edges(emu_ctx, monkeypatch, c):
    """every closed group reads 1; with P perturbed at 0, 63, 64 and the last index exactly the groups that hold them read 0 and out2
    gives their count and the first; group_start = NULL is one group; GA_PAIRING_CHUNK=96 (groups straddle passes) and device-resident
    inputs and outputs give the same bytes"""
    ctx = emu_ctx
    P, Q, gs, a = edge_case(c)
    n = len(P)
    idx = (0, 63, 64, n - 1)
    Pb = perturbed(c, P, a, idx)
    want_bad = np.ones(len(EDGE_SIZES), np.uint8)
    for i in idx:
        want_bad[max(g for g in range(len(EDGE_SIZES)) if gs[g] <= i)] = 0
    assert list(want_bad) == [0, 1, 0, 1, 1, 0]
    for chunk in (None, 96):
        with knobs(monkeypatch, chunk=chunk):
            ok, bad, first = ecc.PairingCheck(ctx, c.name, P, Q, gs)
            assert ok.all() and (bad, first) == (0, NONE_BAD), chunk
            ok, gt, bad, first = ecc.PairingCheck(ctx, c.name, Pb, Q, gs, want_gt=True)
            assert np.array_equal(ok, want_bad) and (bad, first) == (3, 0), (chunk, list(ok))
            ok1, bad1, first1 = ecc.PairingCheck(ctx, c.name, P, Q)
            assert list(ok1) == [1] and (bad1, first1) == (0, NONE_BAD), chunk
            ok1, bad1, first1 = ecc.PairingCheck(ctx, c.name, Pb, Q)
            assert list(ok1) == [0] and (bad1, first1) == (1, 0), chunk
            if chunk is None:
                ref_gt = gt
            else:
                assert np.array_equal(gt, ref_gt)
    dP, dQ = ctx.to_device(Pb), ctx.to_device(Q)
    try:
        with knobs(monkeypatch, chunk=96):
            d_ok, d_gt, bad, first = ecc.PairingCheck(ctx, c.name, dP, dQ, gs, want_gt=True, on_device=True)
        try:
            assert np.array_equal(d_ok.to_host((len(EDGE_SIZES),), np.uint8), want_bad) and (bad, first) == (3, 0)
            assert np.array_equal(d_gt.to_host(ref_gt.shape), ref_gt)
        finally:
            d_ok.free()
            d_gt.free()
        ok, bad, first = ecc.PairingCheck(ctx, c.name, dP, dQ, gs)   # device in, host out
        assert np.array_equal(ok, want_bad)
        assert np.array_equal(dP.to_host(Pb.shape), Pb) and np.array_equal(dQ.to_host(Q.shape), Q)
    finally:
        dP.free()
        dQ.free()


# ---- 3. infinity and purity ----------------------------------------------------------------------------------------------------------------
_BAD_POINTS = {}


def bad_points(c):
    """a Q on the twist outside G2, a Q of small order, and ([a]G1 with y + 1) as arrays"""
    if c.cid not in _BAD_POINTS:
        rng = pyref.Xoshiro(0x9A1 + c.cid)
        q = cp.cofactor(c, 1)[1][0]
        x, y = pyref.g1_group(c).mul(c.g1, 12345)
        _BAD_POINTS[c.cid] = (pts_to_arr(c, 1, [cp.random_curve_point(c, 1, rng)])[0], pts_to_arr(c, 1, [cp.torsion_point(c, 1, q, rng)])[0],
                              pts_to_arr(c, 0, [(x, (y + 1) % c.p)])[0])
    return _BAD_POINTS[c.cid]


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_pairing_infinity_and_purity(emu_ctx, c):
    """(0,0) as P, as Q and as both inside a closed group: still 1; a group of only such pairs: 1.  A Q outside G2, a Q of small order
    and a P off the curve, each alone in a group between closed groups: GA_OK, the neighbours read 1, the inputs are unchanged"""
    ctx = emu_ctx
    a, b = list(logs_a(c, 6)), list(logs_b(c, 6))
    a[5], b[5] = closing(c, a[:2], b[:2])   # pairs 0, 1 and 5 close; 2, 3, 4 get an infinity
    P, Q = pairs(c, a, b)
    P[2] = 0
    Q[3] = 0
    P[4] = 0
    Q[4] = 0
    P = np.concatenate([P, P[2:5]])
    Q = np.concatenate([Q, Q[2:5]])
    ok, bad, first = ecc.PairingCheck(ctx, c.name, P, Q, [0, 6, 9])
    assert list(ok) == [1, 1] and (bad, first) == (0, NONE_BAD)

    out_q, small_q, off_p = bad_points(c)
    a, b = list(logs_a(c, 3)), list(logs_b(c, 3))
    a[2], b[2] = closing(c, a[:2], b[:2])
    cP, cQ = pairs(c, a, b)
    g1 = fb.expected_points(c, 0, [5])
    g2 = fb.expected_points(c, 1, [9])
    P = np.concatenate([cP, g1, cP, g1, cP, off_p[None, :], cP])
    Q = np.concatenate([cQ, out_q[None, :], cQ, small_q[None, :], cQ, g2, cQ])
    gs = [0, 3, 4, 7, 8, 11, 12, 15]
    keepP, keepQ = P.copy(), Q.copy()
    ok, gt, bad, first = ecc.PairingCheck(ctx, c.name, P, Q, gs, want_gt=True)
    assert [int(ok[g]) for g in (0, 2, 4, 6)] == [1, 1, 1, 1]
    assert np.array_equal(P, keepP) and np.array_equal(Q, keepQ)
    assert int(ok[3]) == 0   # a Q of small order: a defined "not 1"
    assert bad == int((ok == 0).sum()) and (first == NONE_BAD) == (bad == 0)
    for g in (0, 2, 4, 6):
        assert gt_to_model(c, gt[g]) == pyref.Fp12Ops(c).one


# ---- 4. gt ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_pairing_gt(emu_ctx, c):
    """gt is 1 exactly where ok is 1; gt{(G1, G2)} is not 1 and has order r; gt{([a]P, Q)} = gt{(P, Q)}^a for a 64-bit a; the gt of a
    two-pair group is the product of the two singles -- all in pyref's Fp12"""
    ctx, F12 = emu_ctx, pyref.Fp12Ops(c)
    gs, _, (P, Q, want) = oracle_case(c)
    ok, gt, bad, first = ecc.PairingCheck(ctx, c.name, P, Q, gs, want_gt=True)
    assert np.array_equal(ok, want)
    for g in range(len(want)):
        assert (gt_to_model(c, gt[g]) == F12.one) == bool(want[g]), g

    a = 0xC0FFEE1234567891
    la, lb = logs_a(c, 2), logs_b(c, 2)
    # groups: (G1, G2); (P0, Q0); ([a]P0, Q0); (P1, Q1); (P0, Q0)(P1, Q1)
    P, Q = pairs(c, [1, la[0], a * la[0], la[1], la[0], la[1]], [1, lb[0], lb[0], lb[1], lb[0], lb[1]])
    ok, gt, bad, first = ecc.PairingCheck(ctx, c.name, P, Q, [0, 1, 2, 3, 4, 6], want_gt=True)
    assert not ok.any() and (bad, first) == (5, 0)
    e = [gt_to_model(c, row) for row in gt]
    assert e[0] != F12.one and F12.pow(e[0], c.r) == F12.one
    assert e[2] == F12.pow(e[1], a)
    assert e[4] == F12.mul(e[1], e[3])


# ---- 5. errors -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_pairing_errors(emu_ctx, c):
    """every GA_ERR_INVALID of include/gnark_amd.h, each followed by a good call on the same context with the right answer;
    n_groups = 0 is GA_OK and touches nothing"""
    ctx, lib, h = emu_ctx, emu_ctx.lib, emu_ctx.handle
    a, b = list(logs_a(c, 4)), list(logs_b(c, 4))
    a[3], b[3] = closing(c, a[1:3], b[1:3])
    P, Q = pairs(c, a, b)
    n = 4
    ok = np.full(2, 0xAB, np.uint8)
    out2 = (C.c_uint64 * 2)(7, 7)
    u64 = lambda *v: np.array(v, np.uint64)
    good = u64(0, 1, 4)
    p = lambda x: x.ctypes.data
    bad = [
        (h, 7, p(P), p(Q), n, p(good), 2, 0, p(ok), None, out2),                      # curve
        (h, c.cid, None, p(Q), n, p(good), 2, 0, p(ok), None, out2),                  # null P, n > 0
        (h, c.cid, p(P), None, n, p(good), 2, 0, p(ok), None, out2),                  # null Q, n > 0
        (h, c.cid, p(P), p(Q), n, p(good), 2, 0, p(ok), None, None),                  # null out2
        (h, c.cid, p(P), p(Q), n, p(u64(1, 1, 4)), 2, 0, p(ok), None, out2),          # group_start[0] != 0
        (h, c.cid, p(P), p(Q), n, p(u64(0, 3, 2, 4)), 3, 0, p(ok), None, out2),       # decreasing
        (h, c.cid, p(P), p(Q), n, p(u64(0, 1, 3)), 2, 0, p(ok), None, out2),          # does not end at n
        (h, c.cid, p(P), p(Q), n, None, 2, 0, p(ok), None, out2),                     # NULL group_start, n_groups != 1
        (h, c.cid, p(P), p(Q), (1 << 32) + 1, p(u64(0, 1, (1 << 32) + 1)), 2, 0, p(ok), None, out2),   # n above 2^32
    ]
    for args in bad:
        assert lib.ga_pairing_check(*args) == -1, args[1:8]   # GA_ERR_INVALID
        assert args[1] == 7 or b"ga_pairing_check" in lib.ga_last_error()
        assert (ok == 0xAB).all() and list(out2) == [7, 7]
        got, nbad, first = ecc.PairingCheck(ctx, c.name, P, Q, good)
        assert list(got) == [0, 1] and (nbad, first) == (1, 0)
    assert lib.ga_pairing_check(h, c.cid, None, None, 0, None, 0, 0, p(ok), None, out2) == 0
    assert (ok == 0xAB).all() and list(out2) == [7, 7]
    assert lib.ga_pairing_check(h, c.cid, p(P), p(Q), n, p(good), 2, 0, p(ok), None, out2) == 0
    assert list(ok) == [0, 1] and list(out2) == [1, 0]
    # no pairs at all: every group is empty, hence 1
    assert lib.ga_pairing_check(h, c.cid, None, None, 0, p(u64(0, 0, 0)), 2, 0, p(ok), None, out2) == 0
    assert list(ok) == [1, 1] and list(out2) == [0, NONE_BAD]


# ---- 6. the verifier -----------------------------------------------------------------------------------------------------------------------
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def proof_of(c, t, lib):
    """the oracle's (Ar, Bs, Krs, commitments, pok) as a groth16.Proof"""
    ar, bs, krs = t[0], t[1], t[2]
    coms = list(t[3]) if len(t) > 3 and t[3] else []
    pok = t[4] if len(t) > 4 else None
    return groth16.Proof(c.cid, pts_to_arr(c, 0, [ar])[0], pts_to_arr(c, 1, [bs])[0], pts_to_arr(c, 0, [krs])[0], lib,
                         pts_to_arr(c, 0, coms) if coms else None, pts_to_arr(c, 0, [pok])[0] if coms else None)


def vk_of(c, vk, pacc=()):
    keys = [(pts_to_arr(c, 1, [vk.commitment_g2])[0], pts_to_arr(c, 1, [s])[0]) for s in vk.commitment_g2_sigma_neg]
    return g16_verify.VerifyingKey(c.cid, pts_to_arr(c, 0, [vk.alpha1])[0], pts_to_arr(c, 1, [vk.beta2])[0], pts_to_arr(c, 1, [vk.gamma2])[0],
                                   pts_to_arr(c, 1, [vk.delta2])[0], pts_to_arr(c, 0, vk.K), keys, [list(x) for x in pacc])


def test_verify_bellman_tuples(emu_ctx):
    """backend/groth16/bellman_test.go:26-84 from tests/golden/bellman_bls12381.json: Verify accepts exactly the six tuples marked ok;
    the key is read by VerifyingKey.ReadFrom from the blob"""
    ctx, c = emu_ctx, BLS12_381
    t = json.load(open(os.path.join(GOLD, "bellman_bls12381.json")))["tuples"]
    assert len(t) == 12 and sum(x["ok"] for x in t) == 6
    got = []
    for x in t:
        vkb, prb, inb = base64.b64decode(x["vk"]), base64.b64decode(x["proof"]), base64.b64decode(x["inputs"])
        vk, used = g16_verify.VerifyingKey.ReadFrom(c.name, vkb, lib=ctx.lib)
        assert set(vkb[used:]) <= {0} and vk.nb_commitments == 0
        proof = proof_of(c, (pyref.g1_decompress(c, prb[:48]), pyref.g2_decompress(c, prb[48:144]), pyref.g1_decompress(c, prb[144:192])), ctx.lib)
        pw = [int.from_bytes(inb[i:i + 32], "big") for i in range(0, len(inb), 32)]
        got.append(g16_verify.Verify(ctx, vk, proof, pw))
    assert got == [x["ok"] for x in t]


_CIRCUITS = {}


def circuits(c):
    """the oracle's keys and proofs of test_oracle_verifier_accepts_oracle_proofs_and_rejects_tampering: the cubic circuit and the
    two-commitment circuit, each as (vk, pacc, proof tuple, public witness)"""
    if c.cid not in _CIRCUITS:
        rng = pyref.Xoshiro(0xBE11)
        cs, w = pyref.cubic_r1cs(), pyref.cubic_witness(3)
        pk, vk, _ = pyref.groth16_setup(c, cs, [rng.field(c.r) for _ in range(5)])
        r, s = rng.field(c.r), rng.field(c.r)
        cubic = (vk, [], pyref.proof_read(c, pyref.proof_bytes(c, *pyref.groth16_prove(pk, cs, w, r, s)))[:5], w[1:cs.nb_public], pk, cs)
        cs2 = pyref.commit_r1cs()
        pk2, vk2, _ = pyref.groth16_setup(c, cs2, [rng.field(c.r) for _ in range(8)])
        w2 = pyref.commit_solve(c, cs2, 5, 7, lambda i, ww: pyref.commitment_hint(pk2, cs2, i, ww)[1])
        proof2 = pyref.proof_read(c, pyref.proof_bytes(c, *pyref.groth16_prove_bsb22(pk2, cs2, w2, r, s)))[:5]
        commit = (vk2, pyref.vk_public_and_commitment_committed(cs2), proof2, w2[1:cs2.nb_public])
        _CIRCUITS[c.cid] = (cubic, commit)
    return _CIRCUITS[c.cid]


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_verify_oracle_proofs_and_tampering(emu_ctx, c):
    """Verify accepts the oracle's proofs for the cubic circuit and for the two-commitment circuit and rejects a wrong public input,
    a proof point moved off its value and a tampered commitment"""
    ctx, G1 = emu_ctx, pyref.g1_group(c)
    cubic, commit = circuits(c)
    vk, pacc, proof, pw = cubic[:4]
    k = vk_of(c, vk, pacc)
    assert g16_verify.Verify(ctx, k, proof_of(c, proof, ctx.lib), pw)
    assert not g16_verify.Verify(ctx, k, proof_of(c, proof, ctx.lib), [(pw[0] + 1) % c.r])
    assert not g16_verify.Verify(ctx, k, proof_of(c, (G1.add(proof[0], c.g1),) + tuple(proof[1:]), ctx.lib), pw)
    assert not g16_verify.Verify(ctx, k, proof_of(c, proof, ctx.lib), list(pw) + [1])   # (one public input too many: an error in the reference)
    vk, pacc, proof, pw = commit
    k = vk_of(c, vk, pacc)
    assert g16_verify.Verify(ctx, k, proof_of(c, proof, ctx.lib), pw)
    assert not g16_verify.Verify(ctx, k, proof_of(c, proof, ctx.lib), [(pw[0] + 1) % c.r])
    bad = (proof[0], proof[1], proof[2], [G1.add(proof[3][0], c.g1), proof[3][1]], proof[4])
    assert not g16_verify.Verify(ctx, k, proof_of(c, bad, ctx.lib), pw)
    # the same through VerifyMany: two groups per proof
    got = g16_verify.VerifyMany(ctx, k, [proof_of(c, proof, ctx.lib), proof_of(c, bad, ctx.lib), proof_of(c, proof, ctx.lib)], [pw, pw, pw])
    assert list(got) == [True, False, True]
    e = k.Precompute(ctx)
    assert e.shape == (12 * c.fp_limbs,) and gt_to_model(c, e) != pyref.Fp12Ops(c).one


_MANY = {}


def cubic_proofs(c, n):
    """n proofs of the cubic circuit under the key of circuits(c), for x = 3, 4, ...: (proof tuple, public witness) each"""
    if c.cid not in _MANY:
        _MANY[c.cid] = []
    have = _MANY[c.cid]
    vk, _, _, _, pk, cs = circuits(c)[0]
    rng = pyref.Xoshiro(0x3A97 + c.cid)
    for _ in range(2 * len(have)):
        rng.field(c.r)
    while len(have) < n:
        w = pyref.cubic_witness(3 + len(have))
        have.append((pyref.groth16_prove(pk, cs, w, rng.field(c.r), rng.field(c.r))[:3], w[1:cs.nb_public]))
    return vk, have[:n]


def tamper(c, proof, pw, how):
    G1 = pyref.g1_group(c)
    if how == 0:
        return proof, [(pw[0] + 1) % c.r]
    if how == 1:
        return (G1.add(proof[0], c.g1), proof[1], proof[2]), pw
    return (proof[0], proof[1], G1.neg(proof[2])), pw


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_verify_many(emu_ctx, c):
    """9 cubic proofs, proofs 0, 4 and 8 tampered in three different ways: VerifyMany returns exactly that pattern, which is
    pyref.groth16_verify proof by proof"""
    ctx = emu_ctx
    vk, items = cubic_proofs(c, 9)
    items = [tamper(c, pr, pw, {0: 0, 4: 1, 8: 2}[i]) if i in (0, 4, 8) else (pr, pw) for i, (pr, pw) in enumerate(items)]
    want = [pyref.groth16_verify(c, vk, pr, pw) for pr, pw in items]
    assert want == [i not in (0, 4, 8) for i in range(9)]
    got = g16_verify.VerifyMany(ctx, vk_of(c, vk), [proof_of(c, pr, ctx.lib) for pr, _ in items], [pw for _, pw in items])
    assert got.dtype == bool and list(got) == want


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_batch_verify(emu_ctx, c):
    """BatchVerify on 8 good proofs is true; with any one of them tampered it is false, under replayed r_i and under a second seed;
    a key with commitments is a ValueError"""
    ctx = emu_ctx
    vk, items = cubic_proofs(c, 8)
    k = vk_of(c, vk)
    proofs, pws = [proof_of(c, pr, ctx.lib) for pr, _ in items], [pw for _, pw in items]
    for seed in (1, 2):
        assert g16_verify.BatchVerify(ctx, k, proofs, pws, np.random.default_rng(seed)) is True
        for i in range(8):
            pr, pw = tamper(c, items[i][0], items[i][1], i % 3)
            bad_p, bad_w = list(proofs), list(pws)
            bad_p[i], bad_w[i] = proof_of(c, pr, ctx.lib), pw
            assert g16_verify.BatchVerify(ctx, k, bad_p, bad_w, np.random.default_rng(seed)) is False, (seed, i)
    vk2, pacc = circuits(c)[1][:2]
    with pytest.raises(ValueError):
        g16_verify.BatchVerify(ctx, vk_of(c, vk2, pacc), [], [], np.random.default_rng(1))


@pytest.mark.parametrize("name", ["bn254_nocommit", "bn254_commit", "bls12381_nocommit", "bls12381_commit"])
def test_verifying_key_read_from(emu_lib, name):
    """VerifyingKey.ReadFrom on the four golden vk files: every field equals pyref.vk_read's"""
    c = BN254 if name.startswith("bn254") else BLS12_381
    raw = open(os.path.join(GOLD, "vk_blank_groth16_%s.bin" % name), "rb").read()
    want, pacc, beta1, delta1, used = pyref.vk_read(c, raw)
    vk, got_used = g16_verify.VerifyingKey.ReadFrom(c.name, raw, lib=emu_lib)
    assert got_used == used and vk.curve == c.cid
    for group, got, exp in ((0, vk.alpha1, want.alpha1), (0, vk.beta1, beta1), (0, vk.delta1, delta1), (1, vk.beta2, want.beta2),
                            (1, vk.gamma2, want.gamma2), (1, vk.delta2, want.delta2)):
        assert np.array_equal(got, pts_to_arr(c, group, [exp])[0])
    assert np.array_equal(vk.K, pts_to_arr(c, 0, want.K))
    assert vk.PublicAndCommitmentCommitted == pacc and len(vk.CommitmentKeys) == len(want.commitment_g2_sigma_neg)
    for (g, sneg), exp in zip(vk.CommitmentKeys, want.commitment_g2_sigma_neg):
        assert np.array_equal(g, pts_to_arr(c, 1, [want.commitment_g2])[0]) and np.array_equal(sneg, pts_to_arr(c, 1, [exp])[0])

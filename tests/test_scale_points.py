"""Per-point scalar multiplication (ga_scale_points, gnark_amd/csrc/scale_points.hip.h: the ScalarMultiplication loops of the Groth16
MPC ceremony, backend/groth16/<curve>/mpcsetup) on the functional emulation.  Every case is a function of a context;
tests/test_scale_points_gpu.py runs the same cases on the device.  Inputs are P_i = [a_i]G with known a_i, expected outputs are
[a_i s_i mod r]G from test_fixed_base.expected_points; every comparison is exact, on affine bytes."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

import pyref
import test_fixed_base as fb
from gnark_amd import _lib, ecc
from gnark_amd._lib import GnarkAmdError
from gnark_amd.device import affine_words
from helpers import BLS12_381, BN254, fr_to_arr, pts_to_arr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = [BN254, BLS12_381]
SIZES = fb.SIZES   # (1, 2, 63, 64, 65, 257, 1000): the wave and workgroup edges
MODES = ["each", "one", "powers", "powers-first-c"]


# ---- the model: signed 4-bit digits, and which scalars leave the fast loop ------------------------------------------------------------
def digits(s):
    """the recoding of scale_points.hip.h: digits in [-8, 8], 64 windows and the carry-out digit"""
    out, carry = [], 0
    for w in range(64):
        d = ((s >> (4 * w)) & 15) + carry
        carry = 1 if d > 8 else 0
        out.append(d - 16 * carry)
    out.append(carry)
    assert sum(d << (4 * w) for w, d in enumerate(out)) == s and all(-8 <= d <= 8 for d in out)
    return out


def hits_exception(s, r):
    """True when the windowed loop on a point P of prime order r meets an exceptional addition: a prefix m of the digits with
    16 m = +-d (mod r) for the next digit d (the condition does not depend on P: [16 m a]G = +-[d a]G iff 16 m = +-d for a != 0)"""
    ds = digits(s)
    top = max(w for w, d in enumerate(ds) if d)
    m = ds[top]
    for w in range(top - 1, -1, -1):
        m *= 16
        d = ds[w]
        if d and ((m - d) % r == 0 or (m + d) % r == 0):
            return True
        m += d
    return m % r == 0


def test_digit_model():
    """the recoding at its corners, and the one scalar family below r that flags an honest lane: r - 2 (prefix r - 1, digit -1)"""
    for c in CURVES:
        r = c.r
        for s in (r - 1, r - 2, 8, 9, 1 << 252, int("8" * 63, 16), int("f" * 63, 16), 0xF << 248):
            digits(s)
        assert digits(int("8" * 63, 16))[:64] == [8] * 63 + [0]
        assert digits(int("f" * 63, 16))[:64] == [-1] + [0] * 62 + [1]
        assert digits(0xF << 248)[62:] == [-1, 1, 0]               # the top digit comes from the carry alone
        assert hits_exception(r - 2, r) and not hits_exception(r - 1, r) and not hits_exception(1, r)


# ---- inputs, shared by every case ---------------------------------------------------------------------------------------------------
_LOGS = {}


def logs(c, n=1000):
    """a_i: the discrete logs of the input points, the same prefix for every size"""
    if c.cid not in _LOGS:
        rng = pyref.Xoshiro(0x5CA1E + c.cid)
        _LOGS[c.cid] = [rng.field(c.r - 1) + 1 for _ in range(1000)]
    return _LOGS[c.cid][:n]


def points(c, group, n):
    return fb.expected_points(c, group, logs(c, n))


def rand_scalars(c, n, seed=0):
    rng = pyref.Xoshiro(0x5CA1A5 + 31 * seed + c.cid)
    return [rng.field(c.r - 1) + 1 for _ in range(1000)][:n]


def expect(c, group, a, s):
    return fb.expected_points(c, group, [x * y % c.r for x, y in zip(a, s)])


def canon(c, ks):
    return fr_to_arr(c, ks, mont=False)


class knobs:
    """GA_SCALE_CHUNK / GA_SCALE_WINDOW for the calls inside the block (read once per entry point)"""

    def __init__(self, monkeypatch, chunk=None, window=None):
        self.mp, self.env = monkeypatch, {"GA_SCALE_CHUNK": chunk, "GA_SCALE_WINDOW": window}

    def __enter__(self):
        for k, v in self.env.items():
            if v is None:
                self.mp.delenv(k, raising=False)
            else:
                self.mp.setenv(k, str(v))

    def __exit__(self, *a):
        for k in self.env:
            self.mp.delenv(k, raising=False)


def mode_case(c, n, mode):
    """(keyword arguments of ScalePoints, the scalar every lane is multiplied by)"""
    if mode == "each":
        s = rand_scalars(c, n)
        return dict(scalars=canon(c, s)), s
    if mode == "one":
        s = rand_scalars(c, 1, seed=1)[0]
        return dict(scalar=s), [s] * n
    t = rand_scalars(c, 1, seed=2)[0]
    if mode == "powers":
        return dict(powers=(1, t)), [pow(t, i, c.r) for i in range(n)]
    cc = rand_scalars(c, 1, seed=3)[0]
    return dict(powers=(cc, t), first=n - 1), [cc * pow(t, n - 1 + i, c.r) % c.r for i in range(n)]


# ---- 1. three modes against known logs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_scale_points_modes(emu_ctx, c, group, mode, sizes=None):
    """n in {1, 2, 63, 64, 65, 257, 1000} (G2 up to 257 on the emulation), random full-width scalars: GA_SCALE_EACH, GA_SCALE_ONE,
    GA_SCALE_POWERS with (first, c) = (0, 1) and (n - 1, random).  redone == 0 in every run -- the fast loop carried the result --
    after the model has confirmed on the CPU that none of the committed scalars meets an exceptional addition"""
    if sizes is None:
        sizes = SIZES if group == 0 else tuple(n for n in SIZES if n <= 257)
    for n in sizes:
        kw, s = mode_case(c, n, mode)
        assert not any(hits_exception(k, c.r) for k in set(s))
        got, redone = ecc.ScalePoints(emu_ctx, c.name, group, points(c, group, n), **kw)
        want = expect(c, group, logs(c, n), s)
        assert got.shape == want.shape
        bad = np.where((got != want).any(axis=1))[0]
        assert bad.size == 0, (n, mode, bad[:8])
        assert redone == 0, (n, mode, redone)


# ---- 2. edge scalars ----------------------------------------------------------------------------------------------------------------
def edge_scalars(c):
    r = c.r
    return [0, 1, 2, 7, 8, 9, 15, 16, r - 1, r - 2] + [1 << k for k in (3, 4, 63, 64, 127, 252)] + [
        int("8" * 63, 16), int("f" * 63, 16),   # the largest all-8-nibble and all-0xF-nibble values below r
        0xF << 248]                             # nibble 62 = 0xF, nibble 63 = 0: the top digit is the carry


@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "montgomery"])
@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_scale_points_edge_scalars(emu_ctx, c, group, mont, n=64):
    """every edge scalar on every point of a 64-point vector, canonical and Montgomery; redone is what the model says: n for r - 2
    (acc = -P meets the digit -1: a doubling in the addition), 0 for everything else; then all of them side by side in one vector.
    r itself, canonical, is not below r: it is reduced, like any 256-bit integer (include/gnark_amd.h), so every output is (0,0)"""
    P, a = points(c, group, n), logs(c, n)
    for s in edge_scalars(c):
        want = expect(c, group, a, [s] * n)
        flagged = n if s and hits_exception(s, c.r) else 0
        got, redone = ecc.ScalePoints(emu_ctx, c.name, group, P, scalar=fr_to_arr(c, [s], mont=mont)[0], montgomery=mont)
        assert np.array_equal(got, want) and redone == flagged, (hex(s), mont, redone)
    each = edge_scalars(c)
    got, redone = ecc.ScalePoints(emu_ctx, c.name, group, P[:len(each)], fr_to_arr(c, each, mont=mont), montgomery=mont)
    assert np.array_equal(got, expect(c, group, a, each)) and redone == 1   # (r - 2 alone)
    if not mont:
        rr = np.array([[(c.r >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]], dtype=np.uint64)
        got, redone = ecc.ScalePoints(emu_ctx, c.name, group, P, scalar=rr[0])
        assert not got.any() and redone == 0
        got, redone = ecc.ScalePoints(emu_ctx, c.name, group, P[:8], np.repeat(rr, 8, axis=0))
        assert not got.any() and redone == 0


# ---- 3. exceptional points ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_scale_points_infinities_and_equal_points(emu_ctx, c, group, n=64):
    """(0,0) at positions 0, 13 and n - 1 stays (0,0) and is not counted; all inputs the same point; one honest lane forced through
    the redo path (scalar r - 2) leaves its neighbours alone and counts once"""
    a, s = logs(c, n), rand_scalars(c, n)
    P, want = points(c, group, n).copy(), expect(c, group, a, s).copy()
    for j in (0, 13, n - 1):
        P[j] = 0
        want[j] = 0
    got, redone = ecc.ScalePoints(emu_ctx, c.name, group, P, canon(c, s))
    assert np.array_equal(got, want) and redone == 0
    same = np.repeat(points(c, group, 1), n, axis=0)
    got, redone = ecc.ScalePoints(emu_ctx, c.name, group, same, canon(c, s))
    assert np.array_equal(got, expect(c, group, [a[0]] * n, s)) and redone == 0
    s2 = list(s)
    s2[17] = c.r - 2
    got, redone = ecc.ScalePoints(emu_ctx, c.name, group, points(c, group, n), canon(c, s2))
    assert np.array_equal(got, expect(c, group, a, s2)) and redone == 1


def test_scale_points_order3_point(emu_ctx):
    """the order-3 point of BLS12-381 G1 with scalars 1, 2, 3, 4 (and 0): P, -P, infinity, P, (0,0) -- through the exact path,
    redone = the lanes with a non-zero scalar; between honest neighbours, which stay on the fast path"""
    c = BLS12_381
    Gp, T = pyref.g1_group(c), fb.order3_point()
    ks = [1, 2, 3, 4, 0]
    a, s = logs(c, 8), rand_scalars(c, 8)
    P = np.concatenate([points(c, 0, 4), pts_to_arr(c, 0, [T] * len(ks)), points(c, 0, 8)[4:]])
    want = np.concatenate([expect(c, 0, a[:4], s[:4]), pts_to_arr(c, 0, [Gp.mul(T, k % 3) for k in ks]), expect(c, 0, a[4:], s[4:])])
    assert np.array_equal(want[4], want[7]) and not want[6].any() and not want[8].any() and not np.array_equal(want[4], want[5])
    got, redone = ecc.ScalePoints(emu_ctx, c.name, 0, P, canon(c, s[:4] + ks + s[4:]))
    assert np.array_equal(got, want) and redone == 4


# ---- 4. chunks and windows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,group", [(BN254, 0), (BLS12_381, 0), (BN254, 1)], ids=["bn254-G1", "bls12-381-G1", "bn254-G2"])
def test_scale_points_chunks_and_plain_ladder(emu_ctx, monkeypatch, c, group, n=257):
    """GA_SCALE_CHUNK=96 at n = 257: three chunks, the last one short, the exponents of GA_SCALE_POWERS running across the chunk
    edges; GA_SCALE_WINDOW=0 (the plain ladder) gives the bytes of the default, chunked or not"""
    a, P = logs(c, n), points(c, group, n)
    cases = [mode_case(c, n, m) for m in ("each", "powers-first-c")]
    for kw, s in cases:
        want = expect(c, group, a, s)
        for chunk, window in ((96, None), (None, 0), (96, 0)):
            with knobs(monkeypatch, chunk=chunk, window=window):
                got, redone = ecc.ScalePoints(emu_ctx, c.name, group, P, **kw)
            assert np.array_equal(got, want) and redone == 0, (chunk, window)
    s = rand_scalars(c, n)
    s[100] = c.r - 2   # chunk 1 of 3: the redo list of a chunk, the total of the call
    with knobs(monkeypatch, chunk=96):
        got, redone = ecc.ScalePoints(emu_ctx, c.name, group, P, canon(c, s))
    assert np.array_equal(got, expect(c, group, a, s)) and redone == 1


# ---- 5. placement and purity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_scale_points_placement_and_purity(emu_ctx, monkeypatch, c, group, n=65):
    """host / device points x host / device output, scalars on host and device: equal bytes; a distinct output leaves the input
    byte-identical; out == points gives the bytes of the out-of-place call, on host and on device, in one chunk and in three"""
    ctx, wa = emu_ctx, affine_words(c.cid, group)
    a, s = logs(c, n), rand_scalars(c, n)
    P, want = points(c, group, n), expect(c, group, a, s)
    keep = P.copy()
    d_in, d_s = ctx.to_device(P), ctx.to_device(canon(c, s))
    try:
        for pts in (P, d_in):
            for sc in (canon(c, s), d_s):
                got, _ = ecc.ScalePoints(ctx, c.name, group, pts, sc, n=n)
                assert np.array_equal(got, want)
                d_out, _ = ecc.ScalePoints(ctx, c.name, group, pts, sc, n=n, out_device=True)
                try:
                    assert np.array_equal(d_out.to_host((n, wa)), want)
                finally:
                    d_out.free()
        assert np.array_equal(P, keep) and np.array_equal(d_in.to_host((n, wa)), keep)
        for chunk in (None, 24):
            with knobs(monkeypatch, chunk=chunk):
                h = keep.copy()
                got, redone = ecc.ScalePoints(ctx, c.name, group, h, canon(c, s), in_place=True)
                assert got is h and np.array_equal(h, want) and redone == 0
                d = ctx.to_device(keep)
                try:
                    got, redone = ecc.ScalePoints(ctx, c.name, group, d, d_s, n=n, in_place=True)
                    assert got is d and np.array_equal(d.to_host((n, wa)), want) and redone == 0
                finally:
                    d.free()
    finally:
        d_in.free()
        d_s.free()


# ---- 6. the ceremony, replayed ----------------------------------------------------------------------------------------------------------
def ceremony_replay(ctx, c, N, check_all=True):
    """setOne, then SrsCommons.update twice through ScalePoints as INTEGRATION.md maps it, in place on the device; returns the device
    buffer of the updated G1.Tau (the caller frees it) and tau1 tau2"""
    rng = pyref.Xoshiro(0xCE8E + c.cid)
    contrib = [tuple(rng.field(c.r - 1) + 1 for _ in range(3)) for _ in range(2)]
    g1, g2 = fb.gen_arr(c, 0), fb.gen_arr(c, 1)
    vec = {"tau1": (0, 2 * N - 1), "tau2": (1, N), "alpha": (0, N), "beta": (0, N)}
    dev = {k: ctx.to_device(np.repeat(g2 if g else g1, m, axis=0)) for k, (g, m) in vec.items()}
    try:
        for tau, alpha, beta in contrib:
            for k, cc in (("tau1", 1), ("tau2", 1), ("alpha", alpha), ("beta", beta)):
                g, m = vec[k]
                got, redone = ecc.ScalePoints(ctx, c.name, g, dev[k], powers=(cc, tau), n=m, in_place=True)
                assert got is dev[k] and redone == 0
        T = contrib[0][0] * contrib[1][0] % c.r
        A, B = contrib[0][1] * contrib[1][1] % c.r, contrib[0][2] * contrib[1][2] % c.r
        idx = {k: (range(m) if check_all else sorted({0, 1, m // 2, m - 2, m - 1} | {rng.next() % m for _ in range(59)})) for k, (g, m) in vec.items()}
        for k, cc in (("tau1", 1), ("tau2", 1), ("alpha", A), ("beta", B)):
            g, m = vec[k]
            got = dev[k].to_host((m, affine_words(c.cid, g)))[list(idx[k])]
            assert np.array_equal(got, fb.expected_points(c, g, [cc * pow(T, i, c.r) % c.r for i in idx[k]])), k
        # a phase-2 step: Z and PKK stand-ins (the updated AlphaTau / BetaTau vectors) times 1/delta
        dinv = pow(rng.field(c.r - 1) + 1, -1, c.r)
        for k, cc in (("alpha", A), ("beta", B)):
            got, redone = ecc.ScalePoints(ctx, c.name, 0, dev[k], scalar=dinv, n=N, in_place=True)
            sample = list(idx[k])[:64]
            assert redone == 0 and np.array_equal(got.to_host((N, affine_words(c.cid, 0)))[sample],
                                                  fb.expected_points(c, 0, [cc * dinv % c.r * pow(T, i, c.r) % c.r for i in sample])), k
        tau1 = dev.pop("tau1")
        return tau1, T
    finally:
        for b in dev.values():
            b.free()


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_scale_points_ceremony_replay(emu_ctx, c, N=64):
    """N = 64: G1.Tau[i] = [(tau1 tau2)^i]G for i < 2N - 1, G2.Tau likewise for i < N, AlphaTau[i] = [alpha1 alpha2 (tau1 tau2)^i]G,
    BetaTau likewise; then the phase-2 scaling by 1/delta"""
    tau1, _ = ceremony_replay(emu_ctx, c, N)
    tau1.free()


# ---- 7. errors and the ABI ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_scale_points_errors(emu_ctx, monkeypatch, c, n=16):
    """every GA_ERR_INVALID of include/gnark_amd.h, each followed by a valid call that succeeds; n = 0; GA_FAULT_THROW: an error
    code, then the same call with the same bytes"""
    ctx, lib, h = emu_ctx, emu_ctx.lib, emu_ctx.handle
    wa = affine_words(c.cid, 0)
    a, s = logs(c, n), rand_scalars(c, n)
    P, S, want = points(c, 0, n), canon(c, s), expect(c, 0, a, s)
    out = np.full((n, wa), 0xAB, np.uint64)
    red = C.c_uint64(77)
    p = lambda x: x.ctypes.data
    call = lambda *args: lib.ga_scale_points(*args, C.byref(red))
    bad = [
        (h, 7, 0, p(P), n, 0, p(S), 0, 0, p(out)),            # curve
        (h, c.cid, 2, p(P), n, 0, p(S), 0, 0, p(out)),        # group
        (h, c.cid, 0, p(P), n, 3, p(S), 0, 0, p(out)),        # mode
        (h, c.cid, 0, p(P), n, -1, p(S), 0, 0, p(out)),
        (h, c.cid, 0, None, n, 0, p(S), 0, 0, p(out)),        # null pointers with n > 0
        (h, c.cid, 0, p(P), n, 0, None, 0, 0, p(out)),
        (h, c.cid, 0, p(P), n, 0, p(S), 0, 0, None),
        (None, c.cid, 0, p(P), n, 0, p(S), 0, 0, p(out)),
        (h, c.cid, 0, p(P), n, 0, p(S), 1, 0, p(out)),        # first outside GA_SCALE_POWERS
        (h, c.cid, 0, p(P), n, 1, p(S), 5, 0, p(out)),
        (h, c.cid, 0, p(P), n, 1, p(S), 0, _lib.SCALARS_ON_DEVICE, p(out)),   # device scalars outside GA_SCALE_EACH
        (h, c.cid, 0, p(P), n, 2, p(S), 0, _lib.SCALARS_ON_DEVICE, p(out)),
        (h, c.cid, 0, p(P), (1 << 32) + 1, 0, p(S), 0, 0, p(out)),            # n above 2^32: nothing behind the pointers is read
    ]
    for args in bad:
        assert call(*args) == -1, args[1:9]
        assert (out == 0xAB).all()
        got, redone = ecc.ScalePoints(ctx, c.name, 0, P, S)
        assert np.array_equal(got, want) and redone == 0
    assert call(h, c.cid, 0, None, 0, 0, None, 0, 0, None) == 0 and red.value == 0
    assert call(h, c.cid, 0, p(P), 0, 0, p(S), 0, 0, p(out)) == 0 and (out == 0xAB).all()
    assert lib.ga_scale_points(h, c.cid, 0, p(P), n, 0, p(S), 0, 0, p(out), None) == 0 and np.array_equal(out, want)   # redone may be NULL
    got, redone = ecc.ScalePoints(ctx, c.name, 0, np.zeros((0, wa), np.uint64), np.zeros((0, 4), np.uint64))
    assert got.shape == (0, wa) and redone == 0
    for kw in (dict(), dict(scalars=S, scalar=1), dict(scalar=1, powers=(1, 2))):
        with pytest.raises(ValueError):
            ecc.ScalePoints(ctx, c.name, 0, P, **kw)
    try:
        monkeypatch.setenv("GA_FAULT_THROW", "ga_scale_points")
        with pytest.raises(GnarkAmdError, match=r"error -3: out of host memory \(std::bad_alloc\) under ga_scale_points"):
            ecc.ScalePoints(ctx, c.name, 0, P, S)
        monkeypatch.delenv("GA_FAULT_THROW")
        got, redone = ecc.ScalePoints(ctx, c.name, 0, P, S)
        assert np.array_equal(got, want) and redone == 0
    finally:
        monkeypatch.delenv("GA_FAULT_THROW", raising=False)


def test_scale_points_symbol_and_go_binding(emu_lib):
    """the entry point is exported and bound; ga.go calls it and go/IDENTS.json resolves that call against the header"""
    assert "ga_scale_points" in _lib.EXPORTED_SYMBOLS and hasattr(emu_lib, "ga_scale_points")
    assert (_lib.SCALE_EACH, _lib.SCALE_ONE, _lib.SCALE_POWERS) == (0, 1, 2)
    header = open(os.path.join(ROOT, "include", "gnark_amd.h")).read()
    assert "int ga_scale_points(ga_ctx* ctx, int curve, int group, const void* points_affine, size_t n, int mode," in header
    for name, v in (("GA_SCALE_EACH", 0), ("GA_SCALE_ONE", 1), ("GA_SCALE_POWERS", 2)):
        assert re.search(rf"#define {name}\s+{v}\b", header)
    go = open(os.path.join(ROOT, "go", "backend", "accelerated", "mi355x", "internal", "ga", "ga.go")).read()
    assert "func (c *Context) ScalePoints(" in go and "C.ga_scale_points(c.h, C.int(curve), C.int(group), points, C.size_t(n), C.int(mode)," in go
    idents = json.load(open(os.path.join(ROOT, "go", "IDENTS.json")))["resolved"]
    assert ["go/backend/accelerated/mi355x/internal/ga/ga.go", "C.ga_scale_points", "include/gnark_amd.h prototype (11 args)"] in idents


# ---- 8. the unreduced sequence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp2", [False, True], ids=["G1", "G2"])
@pytest.mark.parametrize("curve", ["bn254", "bls12-381"])
def test_scale_points_ladder_bounds(curve, fp2):
    """tools/lazy_bounds.py check_ladder(curve, fp2): dbl29 and add29 alternating on each other's outputs, from canonical and negated
    points, stay 2.5 bits below R' with every subtraction constant and the Fp2 operand limit asserted -- for G1 and G2 of both curves,
    so no group is routed through the exact arithmetic; the table build and the windowed loop are made of exactly those two functions"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import lazy_bounds
    out = lazy_bounds.check_ladder(curve, fp2)
    assert all(v < out["limit"] - 2.5 for k, v in out.items() if k != "limit")
    assert lazy_bounds.check_ladder(curve) == lazy_bounds.check_ladder(curve, False)
    src = open(os.path.join(ROOT, "gnark_amd", "csrc", "scale_points.hip.h")).read()
    build = src[src.index("bool scale_build_table("):src.index("void scale_store_inf(")]
    assert build.count("dbl29<F>(") == 4 and build.count("add29<F>(") == 3 and "f29_" not in build
    loop = src[src.index("scale_points_window_kernel("):src.index("// the plain ladder")]
    assert "dbl29<F>(acc);" in loop and "add29<F>(acc, e);" in loop
    assert loop.count("f29_sub<2>(") == 1 and "f29_sub<" not in loop.replace("f29_sub<2>(", "")   # the negated y is the only other arithmetic

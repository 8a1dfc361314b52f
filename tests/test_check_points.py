"""Batch curve and subgroup checks (ga_check_points, gnark_amd/csrc/check_points.hip.h: G1Affine / G2Affine.IsOnCurve and IsInSubGroup
for a vector) and the checked key reads on the functional emulation.  Every case is a function of a context;
tests/test_check_points_gpu.py runs the same cases on the device.  Expected statuses come from the model (Group.on_curve,
Group.mul(P, r) is None) or from construction ([a]G), never from the library."""
import ctypes as C

import numpy as np
import pytest

import pyref
import test_fixed_base as fb
import test_scale_points as sp
from gnark_amd import _lib, ecc, groth16
from gnark_amd._lib import GnarkAmdError
from gnark_amd.device import affine_words
from helpers import BLS12_381, BN254, fr_to_arr, gen_of, group_of, pts_to_arr

CURVES = [BN254, BLS12_381]
OK, OFF, OUT = ecc.POINT_OK, ecc.POINT_OFF_CURVE, ecc.POINT_NOT_IN_SUBGROUP
NONE_BAD = (1 << 64) - 1
PLANTED = (0, 63, 64, 65, 127, 128, 256)   # wave and workgroup edges, the last lane; GA_CHECK_CHUNK=96 puts 127 and 128 in chunk 1
BN_X0, BLS_X0 = 4965661367192848881, -0xd201000000010000


def cofactor(c, group):
    """h with #E = h r, and its primes below 2^16"""
    if c is BN254:
        return (1, ()) if group == 0 else (2 * c.p - c.r, (10069,))
    x = BLS_X0
    if group == 0:
        return (x - 1) ** 2 // 3, (3, 11, 10177)
    return (x ** 8 - 4 * x ** 7 + 5 * x ** 6 - 4 * x ** 4 + 6 * x ** 3 - 4 * x ** 2 - 4 * x + 13) // 9, (13, 23, 2713, 11953)


def test_cofactor_model():
    """the cofactors above: integers with the listed primes, and [h r]Q = O for a random curve point"""
    for c in CURVES:
        for group in (0, 1):
            h, primes = cofactor(c, group)
            assert all(h % q == 0 for q in primes)
            assert group_of(c, group).mul(random_curve_point(c, group, pyref.Xoshiro(5)), h * c.r) is None


def random_curve_point(c, group, rng):
    """a curve point from a random x: in the subgroup only by accident (never, but for BN254 G1 where every curve point is)"""
    G = group_of(c, group)
    while True:
        if group == 0:
            x = rng.field(c.p)
            y = pyref._sqrt_fp((x * x * x + c.b) % c.p, c.p)
        else:
            x = (rng.field(c.p), rng.field(c.p))
            y = pyref._sqrt_fp2(G.F.add(G.F.mul(G.F.mul(x, x), x), c.b2), c.p)
        if y is not None and G.on_curve((x, y)):
            return (x, y)


def torsion_point(c, group, q, rng):
    """a point of order exactly q: a random curve point into the q-part of the group, then raised by q until the next step is infinity
    (the q-part need not be cyclic: for BLS12-381 G1 [h r / q]Q is already infinity)"""
    G = group_of(c, group)
    N = cofactor(c, group)[0] * c.r
    while N % q == 0:
        N //= q
    while True:
        T = G.mul(random_curve_point(c, group, rng), N)
        if T is None:
            continue
        while G.mul(T, q) is not None:
            T = G.mul(T, q)
        return T


def model_status(c, group, P):
    G = group_of(c, group)
    if not G.on_curve(P):
        return OFF
    return OK if G.mul(P, c.r) is None else OUT


_MIXED = {}


def mixed_vector(c, group, n=257):
    """(points, expected statuses, kinds by index): honest [a_i]G with every kind of the issue planted, the kinds that are OK first
    so that the first bad index is 127"""
    key = (c.cid, group)
    if key in _MIXED:
        return _MIXED[key]
    G, g = group_of(c, group), gen_of(c, group)
    rng = pyref.Xoshiro(0xC4EC + 2 * c.cid + group)
    a = sp.logs(c, n)
    P = sp.points(c, group, n)
    want = np.zeros(n, np.uint8)
    honest = lambda i: G.mul(g, a[i])
    w = affine_words(c.cid, group) // 2            # words per coordinate
    pw = c.fp_limbs
    h, primes = cofactor(c, group)
    kinds = {}
    slots = list(PLANTED) + [129 + 3 * k for k in range(40)]

    def plant(kind, pt=None, raw=None, status=None):
        i = slots.pop(0)
        kinds[i] = kind
        if pt is not None or raw is None:
            P[i] = pts_to_arr(c, group, [pt])[0]
            want[i] = model_status(c, group, pt) if status is None else status
        if raw is not None:
            raw(P[i])
            want[i] = OFF   # by construction: an image that is not below p
        return i

    plant("infinity", None)
    i = slots[0]
    plant("-P", G.neg(honest(i)))
    plant("[r-1]G", G.mul(g, c.r - 1))
    plant("generator", g)
    i = slots[0]
    x, y = honest(i)
    y1 = (y + 1) % c.p if group == 0 else ((y[0] + 1) % c.p, y[1])
    assert plant("y+1", (x, y1)) == 127
    i = slots[0]
    Q = random_curve_point(c, group, rng)
    plant("P+[r]Q", G.add(honest(i), G.mul(Q, c.r)))
    tors = [(q, torsion_point(c, group, q, rng)) for q in primes]
    if tors:
        plant("T%d" % tors[0][0], tors[0][1])
    else:
        plant("P+[r]Q again", G.add(honest(slots[0]), G.mul(random_curve_point(c, group, rng), c.r)))
    assert not [s for s in PLANTED if s in slots]

    def image_p(row):            # x (G2: its A1 half) := the integer p itself, not reduced
        row[w - pw:w] = pyref.to_limbs(c.p, pw)

    def all_ones(row):           # y := all ones
        row[w:2 * w] = 0xFFFFFFFFFFFFFFFF
    plant("x image = p", honest(slots[0]), raw=image_p)
    plant("y image all ones", honest(slots[0]), raw=all_ones)
    plant("random curve point", random_curve_point(c, group, rng))
    for q, T in tors:
        plant("T%d" % q, T)
        plant("P+T%d" % q, G.add(honest(slots[0]), T))
    out = (P, want, kinds)
    # what the model must have said of each kind
    for i, k in kinds.items():
        exp = OK if k in ("infinity", "-P", "[r-1]G", "generator") else OFF if k in ("y+1", "x image = p", "y image all ones") else OUT
        if c is BN254 and group == 0 and exp == OUT:
            exp = OK   # cofactor 1: a curve point is in the group
        assert want[i] == exp, (c.name, group, i, k, want[i])
    _MIXED[key] = out
    return out


def summary(want):
    bad = np.nonzero(want)[0]
    return int((want == OFF).sum()), int((want == OUT).sum()), int(bad[0]) if bad.size else NONE_BAD


class knobs:
    """GA_CHECK_CHUNK / GA_CHECK_NAIVE for the calls inside the block (read once per entry point)"""

    def __init__(self, monkeypatch, chunk=None, naive=None):
        self.mp, self.env = monkeypatch, {"GA_CHECK_CHUNK": chunk, "GA_CHECK_NAIVE": naive}

    def __enter__(self):
        for k, v in self.env.items():
            if v is None:
                self.mp.delenv(k, raising=False)
            else:
                self.mp.setenv(k, str(v))

    def __exit__(self, *a):
        for k in self.env:
            self.mp.delenv(k, raising=False)


# ---- 1. honest vectors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_check_points_honest(emu_ctx, c, group, sizes=fb.SIZES):
    """n in {1, 2, 63, 64, 65, 257, 1000}, points [a_i]G: every status OK, both counts 0, first = UINT64_MAX, and redone == 0 -- the
    fast identity decided every lane"""
    for n in sizes:
        st, off, out, first, redone = ecc.CheckPoints(emu_ctx, c.name, group, sp.points(c, group, n))
        assert st.shape == (n,) and not st.any(), (n, np.nonzero(st)[0][:8])
        assert (off, out, first, redone) == (0, 0, NONE_BAD, 0), n


# ---- 2. a mixed vector ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_check_points_mixed(emu_ctx, c, group):
    """n = 257 with infinity, -P, [r-1]G, the generator, y + 1, P + [r]Q, a torsion point at 0, 63, 64, 65, 127, 128, 256 and images
    that are not reduced, a random curve point, T and P + T for every cofactor prime below 2^16 further on: status bytes, both counts
    and first equal the model; with curve_only every 2 becomes 0"""
    P, want, kinds = mixed_vector(c, group)
    st, off, out, first, redone = ecc.CheckPoints(emu_ctx, c.name, group, P)
    wrong = np.nonzero(st != want)[0]
    assert wrong.size == 0, [(int(i), kinds.get(int(i)), int(st[i]), int(want[i])) for i in wrong[:8]]
    assert (off, out, first) == summary(want) and first == 127
    if c is BN254 and group == 0:
        assert out == 0 and redone == 0
    else:
        assert out >= 3
    only = np.where(want == OUT, OK, want).astype(np.uint8)
    st, off, out, first, redone = ecc.CheckPoints(emu_ctx, c.name, group, P, curve_only=True)
    assert np.array_equal(st, only) and (off, out, first, redone) == summary(only) + (0,)


# ---- 3. fast = naive, in chunks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_check_points_naive_and_chunks(emu_ctx, monkeypatch, c, group):
    """GA_CHECK_NAIVE=1 ([r - 1]P = -P on the plain ladder) and GA_CHECK_CHUNK=96 (three chunks, the last one short, the first bad
    point in chunk 1), separately and together: the bytes and counts of case 2"""
    P, want, kinds = mixed_vector(c, group)
    for chunk, naive in ((96, None), (None, 1), (96, 1)):
        with knobs(monkeypatch, chunk=chunk, naive=naive):
            st, off, out, first, redone = ecc.CheckPoints(emu_ctx, c.name, group, P)
        wrong = np.nonzero(st != want)[0]
        assert wrong.size == 0, (chunk, naive, [(int(i), kinds.get(int(i)), int(st[i]), int(want[i])) for i in wrong[:8]])
        assert (off, out, first) == summary(want), (chunk, naive)


# ---- 4. the exact path ------------------------------------------------------------------------------------------------------------------
def test_check_points_order3_point(emu_ctx, monkeypatch):
    """a point of order 3 on BLS12-381 G1 between honest neighbours: its second doubling is exceptional, the lane goes to the exact
    kernel (redone >= 1) and comes back outside the subgroup; in the naive test too"""
    c = BLS12_381
    P = sp.points(c, 0, 5)
    P[2] = pts_to_arr(c, 0, [fb.order3_point()])[0]
    for naive in (None, 1):
        with knobs(monkeypatch, naive=naive):
            st, off, out, first, redone = ecc.CheckPoints(emu_ctx, c.name, 0, P)
        assert list(st) == [OK, OK, OUT, OK, OK] and (off, out, first) == (0, 1, 2) and redone >= 1, naive


# ---- 5. placement and purity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_check_points_placement_and_purity(emu_ctx, c, group):
    """host and device points x status on the host, on the device and NULL: the same bytes and counts; the input is byte-identical
    afterwards; an honest vector right after the mixed one is clean (no stale count, no stale redo)"""
    ctx, wa = emu_ctx, affine_words(c.cid, group)
    P, want, _ = mixed_vector(c, group)
    n, keep = len(want), P.copy()
    d_in = ctx.to_device(P)
    try:
        for pts in (P, d_in):
            st, *rest = ecc.CheckPoints(ctx, c.name, group, pts, n=n)
            assert np.array_equal(st, want) and tuple(rest[:3]) == summary(want)
            d_st, *rest_d = ecc.CheckPoints(ctx, c.name, group, pts, n=n, status_device=True)
            try:
                assert np.array_equal(d_st.to_host((n,), np.uint8), want) and rest_d == rest
            finally:
                d_st.free()
            none, *rest_n = ecc.CheckPoints(ctx, c.name, group, pts, n=n, status=False)
            assert none is None and rest_n == rest
            st, *clean = ecc.CheckPoints(ctx, c.name, group, sp.points(c, group, 65))
            assert not st.any() and clean == [0, 0, NONE_BAD, 0]
        assert np.array_equal(P, keep) and np.array_equal(d_in.to_host((n, wa)), keep)
    finally:
        d_in.free()


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_check_points_errors(emu_ctx, c, n=16):
    """every GA_ERR_INVALID of include/gnark_amd.h, each followed by a valid call that succeeds; n = 0 gives {0, 0, UINT64_MAX, 0}
    and touches nothing"""
    ctx, lib, h = emu_ctx, emu_ctx.lib, emu_ctx.handle
    P = sp.points(c, 0, n)
    st = np.full(n, 0xAB, np.uint8)
    out4 = (C.c_uint64 * 4)(7, 7, 7, 7)
    p = lambda x: x.ctypes.data
    bad = [
        (h, 7, 0, p(P), n, 0, p(st), out4),                  # curve
        (h, c.cid, 2, p(P), n, 0, p(st), out4),              # group
        (h, c.cid, 0, None, n, 0, p(st), out4),              # null points, n > 0
        (h, c.cid, 0, p(P), n, 0, p(st), None),              # null out4
        (h, c.cid, 0, p(P), (1 << 32) + 1, 0, p(st), out4),  # n above 2^32
    ]
    for args in bad:
        assert lib.ga_check_points(*args) == -1, args[1:3]   # GA_ERR_INVALID
        assert b"ga_check_points" in lib.ga_last_error()
        assert (st == 0xAB).all() and list(out4) == [7, 7, 7, 7]
        got, *rest = ecc.CheckPoints(ctx, c.name, 0, P)
        assert not got.any() and rest == [0, 0, NONE_BAD, 0]
    assert lib.ga_check_points(h, c.cid, 0, None, 0, 0, p(st), out4) == 0
    assert list(out4) == [0, 0, NONE_BAD, 0] and (st == 0xAB).all()
    assert lib.ga_check_points(h, c.cid, 0, p(P), n, 0, p(st), out4) == 0 and not st.any()


def test_check_points_symbols_and_flags(emu_lib):
    """the flag takes a bit no other call uses; the status values are the header's"""
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gnark_amd.h")).read()
    flags = {k: int(v, 16) for k, v in re.findall(r"#define (GA_[A-Z_]+) +(0x[0-9a-f]+)u", hdr) if k != "GA_PLONK_ON_DEVICE"}
    assert flags["GA_CHECK_CURVE_ONLY"] == _lib.CHECK_CURVE_ONLY and list(flags.values()).count(_lib.CHECK_CURVE_ONLY) == 1
    for name, v in (("GA_POINT_OK", OK), ("GA_POINT_OFF_CURVE", OFF), ("GA_POINT_NOT_IN_SUBGROUP", OUT)):
        assert re.search(r"#define %s +%d\b" % (name, v), hdr)
    assert hasattr(emu_lib, "ga_check_points")


# ---- 7. checked key reads -----------------------------------------------------------------------------------------------------------------
def key_case(c):
    """a small key with one commitment (pyref.commit_r1cs), what proves with it, and its three file images"""
    rng = pyref.Xoshiro(0xC4ECED + c.cid)
    cs = pyref.commit_r1cs()
    pk, _, _ = pyref.groth16_setup(c, cs, [rng.field(c.r) for _ in range(5 + len(cs.commitments) + 1)])
    w = pyref.commit_solve(c, cs, 4, 9, lambda i, ww: pyref.commitment_hint(pk, cs, i, ww)[1])
    removed = sorted({j for cm in cs.commitments for j in cm.private_committed} | {cm.commitment_index for cm in cs.commitments})
    A, B, Cc = pyref.r1cs_solve(c, cs, w)
    sol = groth16.Solution(W=fr_to_arr(c, w), A=fr_to_arr(c, A), B=fr_to_arr(c, B), C=fr_to_arr(c, Cc))
    r, s = fr_to_arr(c, [rng.field(c.r)]), fr_to_arr(c, [rng.field(c.r)])
    return pk, cs, removed, sol, r, s, rng


def key_images(pk):
    return {"compressed": pyref.pk_write(pk, raw=False), "raw": pyref.pk_write(pk, raw=True), "dump": pyref.pk_write_dump(pk)}


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_checked_key_reads(emu_ctx, c):
    """ProvingKey.ReadFrom(subgroup_check=True) on a key with a commitment, compressed, raw and dump: the untampered key reads and
    proves to the bytes of the unchecked read; with one point replaced by P + [r]Q (a G2.B point, [beta]2, and on BLS12-381 a G1.A
    point and a commitment basis point -- BN254 G1 has no such point) the UNCHECKED reader accepts the key, which is the gap, and the
    checked one refuses it with GA_ERR_INVALID naming vector and index, in every format; the next checked read of the good bytes
    succeeds; shard 1 of 2 accepts a bad point of shard 0's slice, shard 0 refuses it"""
    import dataclasses
    ctx = emu_ctx
    pk, cs, removed, sol, r, s, rng = key_case(c)
    good = key_images(pk)
    proofs = set()
    for fmt, img in good.items():
        for check in (False, True):
            dpk = groth16.ProvingKey.ReadFrom(ctx, c.name, img, k_remove=removed, subgroup_check=check)
            try:
                assert dpk.bytes_read == len(img)
                proofs.add(groth16.Prove(dpk, sol, cs.nb_public, r, s).raw().tobytes())
            finally:
                dpk.FreeGPUResources()
    assert len(proofs) == 1
    G1, G2 = pyref.g1_group(c), pyref.g2_group(c)
    out1 = lambda P: G1.add(P, G1.mul(random_curve_point(c, 0, rng), c.r))
    out2 = lambda P: G2.add(P, G2.mul(random_curve_point(c, 1, rng), c.r))
    swap = lambda v, i, P: v[:i] + [P] + v[i + 1:]
    assert len(pk.B2) >= 2 and len(pk.A) >= 3 and len(pk.commitment_keys[0][0]) >= 1
    j2, ja = len(pk.B2) - 1, 2
    cases = [(dataclasses.replace(pk, B2=swap(pk.B2, j2, out2(pk.B2[j2]))), r"point %d of G2\.B" % j2),
             (dataclasses.replace(pk, beta2=out2(pk.beta2)), r"point 0 of \[beta\]2")]
    if c is BLS12_381:
        basis, sigma = pk.commitment_keys[0]
        cases += [(dataclasses.replace(pk, A=swap(pk.A, ja, out1(pk.A[ja]))), r"point %d of G1\.A" % ja),
                  (dataclasses.replace(pk, commitment_keys=[(swap(basis, 0, out1(basis[0])), sigma)]), r"point 0 of a commitment key's Basis\b")]
    for bad_pk, where in cases:
        for fmt, img in key_images(bad_pk).items():
            dpk = groth16.ProvingKey.ReadFrom(ctx, c.name, img, k_remove=removed)   # the unchecked reader takes it: the gap
            dpk.FreeGPUResources()
            with pytest.raises(GnarkAmdError, match=r"error -1: .*" + where + r" is not in the prime-order subgroup"):
                groth16.ProvingKey.ReadFrom(ctx, c.name, img, k_remove=removed, subgroup_check=True)
            dpk = groth16.ProvingKey.ReadFrom(ctx, c.name, good[fmt], k_remove=removed, subgroup_check=True)
            dpk.FreeGPUResources()
    # a dump is raw memory that nothing validates today: a point off the curve
    x, y = pk.A[ja]
    img = pyref.pk_write_dump(dataclasses.replace(pk, A=swap(pk.A, ja, (x, (y + 1) % c.p))))
    groth16.ProvingKey.ReadFrom(ctx, c.name, img, k_remove=removed).FreeGPUResources()
    with pytest.raises(GnarkAmdError, match=r"point %d of G1\.A is not on the curve" % ja):
        groth16.ProvingKey.ReadFrom(ctx, c.name, img, k_remove=removed, subgroup_check=True)
    # shards: the first point of G2.B belongs to shard 0 of 2
    bad0 = key_images(dataclasses.replace(pk, B2=swap(pk.B2, 0, out2(pk.B2[0]))))
    for fmt, img in bad0.items():
        dpk = groth16.ProvingKey.ReadFrom(ctx, c.name, img, k_remove=removed, shard=(1, 2), subgroup_check=True)
        dpk.FreeGPUResources()
        with pytest.raises(GnarkAmdError, match=r"point 0 of G2\.B"):
            groth16.ProvingKey.ReadFrom(ctx, c.name, img, k_remove=removed, shard=(0, 2), subgroup_check=True)

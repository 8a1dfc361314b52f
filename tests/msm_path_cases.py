"""The MSM paths that ordinary inputs never enter: the cases tests/test_msm_paths.py runs on the functional emulation and
tests/test_msm_paths_gpu.py on the device, at the same sizes unless a case says otherwise.  Which lines each case enters is
measured, not assumed: profiles/emu_coverage.txt (tools/emu_coverage.sh).

Every expected value comes from pyref's big-integer group law and known discrete logs: bases are [k_i]G, the expected point is
[sum s_i k_i]G by ONE python multiplication, and the comparison is on canonical affine coordinates.  Nothing is computed through the
library under test.

The five MSM objects (curve x group) are instantiated separately, and the lazy-limb bounds differ per base field, so (a) .. (c) and
(e) run for each of them.

What "exceptional" means here: the lazy sums (msm_lazy.hip.h) add with formulas that are wrong for P + P and P - P; such an addition
leaves ZZ = 0, the sum is flagged and repeated with the complete formulas.  Distinct random bases never meet that, so the inputs
below are built from ONE point."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bls12_377_params  # noqa: E402
import pyref  # noqa: E402
from gnark_amd import ecc  # noqa: E402
from helpers import fr_to_arr, group_of, jac_to_affine_py, pts_to_arr  # noqa: E402

BLS12_377 = bls12_377_params.curve()
OBJECTS = [(pyref.BN254, 0), (pyref.BN254, 1), (pyref.BLS12_381, 0), (pyref.BLS12_381, 1), (BLS12_377, 0)]
OBJECT_IDS = ["bn254-G1", "bn254-G2", "bls12-381-G1", "bls12-381-G2", "bls12-377-G1"]

K0 = 0x0f1e2d3c4b5a69788796a5b4c3d2e1f00112233445566778899aabbccddeeff1
DD = 0x0123456789abcdef0fedcba987654321123456789abcdef00fedcba987654321


def _gen(c, group):
    return c.g1 if group == 0 else c.g2


def gmul(c, group, k):
    return group_of(c, group).mul(_gen(c, group), k % c.r)


@functools.lru_cache(maxsize=None)
def chain(c, group, n):
    """(affine rows, dlogs) of P_i = [K0 + i DD]G, i < n: one multiplication and a chain of python additions, computed once"""
    G = group_of(c, group)
    pts, logs, step = [gmul(c, group, K0)], [K0 % c.r], gmul(c, group, DD)
    while len(pts) < n:
        pts.append(G.add(pts[-1], step))
        logs.append((logs[-1] + DD) % c.r)
    return pts_to_arr(c, group, pts), logs


@functools.lru_cache(maxsize=None)
def one_point(c, group):
    """(row of P, row of -P, k) with P = [k]G"""
    G, k = group_of(c, group), K0 % c.r
    P = gmul(c, group, k)
    return pts_to_arr(c, group, [P])[0], pts_to_arr(c, group, [G.neg(P)])[0], k


def small_scalars(vals):
    """canonical (non-Montgomery) images of integers below 2^64"""
    S = np.zeros((len(vals), 4), dtype=np.uint64)
    S[:, 0] = np.asarray(vals, dtype=np.uint64)
    return S


def affine(c, group, jac):
    return jac_to_affine_py(c, group, jac)


def table_of(ctx, c, group, rows, monkeypatch, table_c=None):
    """a window table, its width forced by GA_TABLE_C while it is planned"""
    if table_c:
        monkeypatch.setenv("GA_TABLE_C", str(table_c))
    try:
        T = ecc.PrecomputedBases(ctx, c.name, group, rows)
    finally:
        if table_c:
            monkeypatch.delenv("GA_TABLE_C")
    if table_c:
        assert T.info()["window_bits"] == table_c, T.info()
    return T


# ---- (a) equal partial sums in one hot bucket --------------------------------------------------------------------------------------
def case_hot_bucket(ctx, c, group, n, monkeypatch, cancel=False, table=True):
    """n copies of ONE point P with scalar 1: every pair lands in the digit-1 bucket of window 0, the task length is 32
    (msm_plan_prepare: want = 1, lo = 32), so the bucket gets ceil(n / 32) partial sums, all of them [32]P but the last.
    n = 600: 19 partials, msm_hot_kernel; n = 17000: 532 partials, msm_vhot_stage1_kernel (parts of 9 equal partials) and
    msm_vhot_stage2_kernel (59 equal results of stage 1).  Each of these block sums meets [32]P + [32]P in its first tree level and
    has to take block_sum29's exact fallback.  cancel: the bases alternate P, -P in blocks of 32, so that neighbouring partials are
    opposite points; what remains is the surplus of one sign.  Raw (ga_msm) and over a window table.
    The route is not visible from outside (ga_profile_read reports stage times, not list lengths): that the hot and very hot lists
    were non-empty and the fallback ran for every object is read off profiles/emu_coverage.txt (msm_reduce.hip.h 29-31, 50-56, 71,
    89-94; msm_lazy.hip.h 137-142)."""
    P, negP, k = one_point(c, group)
    rows = np.tile(P, (n, 1))
    sign = np.ones(n, dtype=np.int64)
    if cancel:
        sign[(np.arange(n) // 32) % 2 == 1] = -1
        rows[sign < 0] = negP
    want = gmul(c, group, int(sign.sum()) * k)
    S = small_scalars([1] * n)
    assert affine(c, group, ecc.MultiExp(ctx, c.name, group, rows, S, montgomery=False)) == want, ("ga_msm", n, cancel)
    if table:
        T = table_of(ctx, c, group, rows, monkeypatch)
        try:
            for run in range(2):   # (the second run knows the table as degenerate)
                assert affine(c, group, T.MultiExp(S, montgomery=False)) == want, ("ga_msm_table_run", n, cancel, run)
        finally:
            T.free()


# ---- (b) equal running sums in the lazy window reduction --------------------------------------------------------------------------
def case_equal_running_sums(ctx, c, group, table_c, monkeypatch, every_second=False):
    """GA_REDUCE_LAZY_MIN=0, one point P, scalars 1 .. half of a table of width table_c (half = 2^(table_c-1) buckets, groups of 2): every
    bucket holds exactly P, every group's running sum is [2]P and its local sum [3]P.  The per-bit tree sums of
    msm_bit_partial_kernel add 32 equal points per chunk of 64 groups, and msm_segment_sum29_kernel adds the equal results of the
    half / 128 chunks (table_c = 10: four): both take block_sum29's exact fallback.  every_second: only the even digits, so every
    second bucket is empty.  The raw MSM of the same shape (1024 points on the digits 1 .. half of the planned width) has one
    chunk per window: the bit sums again.  Expected [sum of the scalars]P."""
    P, _, k = one_point(c, group)
    monkeypatch.setenv("GA_REDUCE_LAZY_MIN", "0")
    half = 1 << (table_c - 1)
    digits = list(range(2, half + 1, 2)) if every_second else list(range(1, half + 1))
    rows, S = np.tile(P, (len(digits), 1)), small_scalars(digits)
    T = table_of(ctx, c, group, rows, monkeypatch, table_c)
    try:
        assert affine(c, group, T.MultiExp(S, montgomery=False)) == gmul(c, group, sum(digits) * k), ("table", table_c, every_second)
    finally:
        T.free()
    n = 1024
    rc = ecc.plan(c.name, group, n, lib=ctx.lib)[0]
    rhalf = 1 << (rc - 1)
    assert n % rhalf == 0 and n // rhalf >= 2, (n, rc)
    step = 2 if every_second else 1
    digits = [step + (i * step) % rhalf for i in range(n)]   # 1 .. rhalf, or 2, 4 .. rhalf, each equally often
    assert max(digits) == rhalf and min(digits) == step
    got = ecc.MultiExp(ctx, c.name, group, np.tile(P, (n, 1)), small_scalars(digits), montgomery=False)
    assert affine(c, group, got) == gmul(c, group, sum(digits) * k), ("raw", rc, every_second)


# ---- (c) the two-level set sum of the exact window reduction ---------------------------------------------------------------------
def carry_only_scalars(c, table_c):
    """two scalars whose TOP window of width table_c holds the signed-digit carry and nothing else: the digit below it is
    2^(table_c-1) + 1 (negative, carries); and the carry chain through every window from the lowest digit up"""
    nwin = c.r.bit_length() // table_c + 1
    a = ((1 << (table_c - 1)) + 1) << (table_c * (nwin - 2))
    b = sum(1 << (table_c * w + table_c - 1) for w in range(nwin - 1)) + 1
    assert a < c.r and b < c.r and (a >> (table_c * (nwin - 1))) == 0 and (b >> (table_c * (nwin - 1))) == 0
    return [a, b]


def case_two_level_exact(ctx, c, group, monkeypatch, n=300, table_c=14, seed=0xC14):
    """a table of width 14 over 300 points: 8192 buckets in one set that is neither big (< GA_REDUCE_LAZY_MIN = 2^14) nor dense
    (19 x 300 pairs), so msm_reduce_plan takes the exact reduction with groups of 2, groups_per_win = 4096 > 2048: the set sum has two
    levels (msm_reduce.hip.h msm_reduce_exact, four segments of 1024 group results, then their sum).  Random full-width scalars with 0, 1,
    r - 1 and the carry-only top window; both scalar forms.
    (No n is PLANNED with width 14: 253, 254 and 255 scalar bits leave a top window of 1 .. 3 bits there, which msm_plan_table
    penalises by 1.25, and 23.75 n + 61440 is above width 13's 20 n + 24576 for every n.  The knob is the only way in.)"""
    rows, logs = chain(c, group, n)
    rng = pyref.Xoshiro(seed + group)
    S = [rng.field(c.r) for _ in range(n)]
    special = [0, 1, c.r - 1] + carry_only_scalars(c, table_c)
    S[3:3 + len(special)] = special
    want = gmul(c, group, sum(s * k for s, k in zip(S, logs)))
    T = table_of(ctx, c, group, rows, monkeypatch, table_c)
    try:
        assert T.info()["windows"] == c.r.bit_length() // table_c + 1
        assert affine(c, group, T.MultiExp(fr_to_arr(c, S))) == want, "Montgomery scalars"
        can = np.array([pyref.to_limbs(v, 4) for v in S], dtype=np.uint64)
        assert affine(c, group, T.MultiExp(can, montgomery=False)) == want, "canonical scalars"
    finally:
        T.free()


# ---- (d) the running-sum group size and the task length, the two knobs no other test sets ------------------------------------------
def group_table_c(group_size):
    """the narrowest table whose single bucket set keeps GA_MSM_GROUP = group_size: msm_reduce_plan halves the group until
    half / group >= 32768"""
    return (32768 * group_size).bit_length()   # half = 2^(c-1) = 32768 * group_size


def case_group_size(ctx, c, group, group_size, monkeypatch, n=2048, min_seg=None, seed=0x6e):
    """GA_MSM_GROUP = group_size over a table just wide enough for the plan to keep it, with the lazy reduction (the default for a set
    this large: msm_combine_set's 2^log_m) and with the exact one (GA_REDUCE_LAZY_MIN above every size: msm_reduce_groups_kernel's
    base * running term with m = group_size).  n known-log points; a quarter of the scalars equal one, so the digit-1 bucket is hot,
    and with min_seg (GA_MSM_MIN_SEG; it is the task length from 2^19 buckets up) that bucket's task count changes."""
    table_c = group_table_c(group_size)
    rows, logs = chain(c, group, n)
    rng = pyref.Xoshiro(seed + group_size)
    S = [1 if i % 4 == 0 else rng.field(c.r) for i in range(n)]
    S[1], S[2] = 0, c.r - 1
    want = gmul(c, group, sum(s * k for s, k in zip(S, logs)))
    Sa = fr_to_arr(c, S)
    T = table_of(ctx, c, group, rows, monkeypatch, table_c)
    try:
        monkeypatch.setenv("GA_MSM_GROUP", str(group_size))
        if min_seg:
            monkeypatch.setenv("GA_MSM_MIN_SEG", str(min_seg))
        assert affine(c, group, T.MultiExp(Sa)) == want, ("lazy reduction", group_size, table_c, min_seg)
        monkeypatch.setenv("GA_REDUCE_LAZY_MIN", str(1 << 40))
        assert affine(c, group, T.MultiExp(Sa)) == want, ("exact reduction", group_size, table_c, min_seg)
    finally:
        for name in ("GA_MSM_GROUP", "GA_MSM_MIN_SEG", "GA_REDUCE_LAZY_MIN"):
            monkeypatch.delenv(name, raising=False)
        T.free()


def case_min_seg_hot_bucket(ctx, min_seg, monkeypatch, c=pyref.BN254, group=0, n=3000):
    """GA_MSM_MIN_SEG on a witness-like vector (nine scalars in ten equal to one, eight distinct bases): the input of
    test_emu_msm_hot_bucket_and_windows, expected by grouping by base.  At this size the knob cannot change the plan: below 2^19
    buckets msm_plan_prepare caps the task length at 32 whatever it says, so the three values check that it is read and harmless.  Where
    it IS the task length -- from 2^19 buckets up -- the callers run case_group_size(.., 16, min_seg=..) beside this."""
    rows, logs = chain(c, group, 8)
    rng = pyref.Xoshiro(5)
    S = [1 if i % 10 else (rng.next() & 0xFFFF) for i in range(n)]
    want = gmul(c, group, sum(s * logs[i % 8] for i, s in enumerate(S)))
    monkeypatch.setenv("GA_MSM_MIN_SEG", str(min_seg))
    try:
        got = ecc.MultiExp(ctx, c.name, group, rows[np.arange(n) % 8], small_scalars(S), montgomery=False)
    finally:
        monkeypatch.delenv("GA_MSM_MIN_SEG")
    assert affine(c, group, got) == want, min_seg


# ---- (e) the exact bucket redo -----------------------------------------------------------------------------------------------------
def case_exact_bucket_redo(ctx, c, group, monkeypatch, n=600):
    """GA_MSM_EXACT_REDO=1 sends every flagged task to msm_accumulate29_redo_kernel (complete formulas, exact arithmetic); all bases
    equal, so every task is flagged.  Random scalars: the buckets of every window are in use."""
    P, _, k = one_point(c, group)
    rng = pyref.Xoshiro(0xE0 + group)
    S = [rng.field(c.r) for _ in range(n)]
    want = gmul(c, group, sum(S) * k)
    rows, Sa = np.tile(P, (n, 1)), fr_to_arr(c, S)
    monkeypatch.setenv("GA_MSM_EXACT_REDO", "1")
    try:
        assert affine(c, group, ecc.MultiExp(ctx, c.name, group, rows, Sa)) == want, "ga_msm"
        T = table_of(ctx, c, group, rows, monkeypatch)
        try:
            assert affine(c, group, T.MultiExp(Sa)) == want, "ga_msm_table_run"
        finally:
            T.free()
    finally:
        monkeypatch.delenv("GA_MSM_EXACT_REDO")


# ---- (f) the point-vector calls: the branches the coverage report showed as never run for one object -------------------------------------
def case_plain_ladder_with_skips(ctx, c, group, monkeypatch, n=24):
    """ga_scale_points on the plain double-and-add ladder (GA_SCALE_WINDOW=0) with (0,0) points and zero scalars in the vector: the lanes
    that scale_points_plain_kernel answers with (0,0) before the ladder, between lanes that run it.  Expected [s_i k_i]G."""
    rows, logs = chain(c, group, n)
    rows = rows.copy()
    rng = pyref.Xoshiro(0xF1 + group)
    S = [rng.field(c.r) for _ in range(n)]
    for i in (0, 7, n - 1):
        S[i] = 0
    for i in (1, 7, 13):
        rows[i] = 0
    want = pts_to_arr(c, group, [None if (s == 0 or not rows[i].any()) else gmul(c, group, s * logs[i]) for i, s in enumerate(S)])
    monkeypatch.setenv("GA_SCALE_WINDOW", "0")
    try:
        got, redone = ecc.ScalePoints(ctx, c.name, group, rows, np.array([pyref.to_limbs(s, 4) for s in S], dtype=np.uint64))
    finally:
        monkeypatch.delenv("GA_SCALE_WINDOW")
    assert np.array_equal(got, want) and redone == 0


def case_to_lagrange_small_order_sum(ctx, c, T, n=8):
    """ga_kzg_to_lagrange_g1 over pairs P, -P, a (0,0) and ONE point T of order 3 (on the curve, outside the subgroup): the inputs sum to
    T, which is what the stages leave at position 0, and [1/n]T on the lazy ladder meets T + 2T: ec_ntt_scale_kernel's complete-formula
    branch; the butterflies that multiply a multiple of T are flagged the same way.  (On BN254 G1, whose cofactor is 1, no such input
    exists.)  For a point outside the subgroup [k]T depends on the INTEGER k, not on k mod r, so the reference is the documented stage
    sequence itself (ec_ntt.hip.h: radix-2 DIF, k = w^(-j 2^s) below r, times 1/n mod r in group 0, 1/n on position 0, bit-reversed
    output) in big integers with pyref's group law, which is complete."""
    G = group_of(c, 0)
    assert G.on_curve(T) and G.mul(T, 3) is None and G.add(T, T) is not None
    a, b, d = (gmul(c, 0, K0 + i * DD) for i in range(3))
    work = [a, G.neg(a), b, None, G.neg(b), T, d, G.neg(d)][:n]
    pts = pts_to_arr(c, 0, work)
    logn = n.bit_length() - 1
    winv, ninv = pow(c.fr_root_of_unity(n), -1, c.r), pow(n, -1, c.r)
    for s in range(logn):
        lm = logn - 1 - s
        for g in range(1 << s):
            for j in range(1 << lm):
                ia = (g << (lm + 1)) + j
                ib = ia + (1 << lm)
                x, y = work[ia], work[ib]
                diff = G.add(x, G.neg(y) if y is not None else None)
                if g == 0 or j != 0:
                    k = pow(winv, j << s, c.r) * (ninv if g == 0 else 1) % c.r
                    diff = G.mul(diff, k) if diff is not None else None
                work[ia], work[ib] = G.add(x, y), diff
    work[0] = G.mul(work[0], ninv)
    assert work[0] == G.mul(T, ninv % 3)
    want = [None] * n
    for i in range(n):
        want[pyref.bitrev(i, logn)] = work[i]
    got = ecc.ToLagrangeG1(ctx, c.name, pts)
    assert np.array_equal(got, pts_to_arr(c, 0, want))


def case_to_lagrange_equal_points(ctx, c, n=16):
    """n copies of one point P: every butterfly is P + P beside P - P, so every lane of ec_ntt_stage_kernel is flagged and redone by
    ec_ntt_exact_kernel.  The inverse transform of a constant vector: out[0] = P, (0,0) elsewhere."""
    P, _, _ = one_point(c, 0)
    want = np.zeros((n, P.shape[0]), dtype=np.uint64)
    want[0] = P
    assert np.array_equal(ecc.ToLagrangeG1(ctx, c.name, np.tile(P, (n, 1))), want)

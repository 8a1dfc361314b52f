"""Groth16 Phase2.Initialize on the device (backend/groth16/<curve>/mpcsetup/phase2.go:150-309): ga_sparse_point_sums
(gnark_amd/csrc/sparse_sums.hip.h: a sparse Fr matrix applied to a vector of points) and ga_lagrange_coeffs (ec_ntt.hip.h: the point
iFFT for G1 and G2) on the functional emulation.  Every case is a function of a context; tests/test_phase2_init_gpu.py runs the same
cases on the device.  Inputs are P_j = [a_j]G with known a_j, the expected row is [sum c_k a_col_k mod r]G from
test_fixed_base.expected_points; every comparison is exact, on affine words."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import oracle
import pyref
import test_fixed_base as fb
import test_scale_points as sp
import test_to_lagrange as tl
from gnark_amd import _lib, ecc
from gnark_amd._lib import GnarkAmdError
from gnark_amd.device import affine_words
from helpers import BLS12_381, BN254, fr_to_arr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = [BN254, BLS12_381]
PAIRS = [(c, g) for c in CURVES for g in (0, 1)]
PAIR_IDS = [f"{c.name}-G{g + 1}" for c, g in PAIRS]
SIZES = fb.SIZES   # (1, 2, 63, 64, 65, 257, 1000)
NPTS = 257


class knobs:
    """GA_SPARSE_CHUNK / GA_SPARSE_SEGMENT / GA_SPARSE_ORDER / GA_EC_NTT_UNIFORM for the calls inside the block (read once per entry point)"""

    def __init__(self, monkeypatch, chunk=None, segment=None, order=None, uniform=None):
        self.mp = monkeypatch
        self.env = {"GA_SPARSE_CHUNK": chunk, "GA_SPARSE_SEGMENT": segment, "GA_SPARSE_ORDER": order, "GA_EC_NTT_UNIFORM": uniform}

    def __enter__(self):
        for k, v in self.env.items():
            if v is None:
                self.mp.delenv(k, raising=False)
            else:
                self.mp.setenv(k, str(v))

    def __exit__(self, *a):
        for k in self.env:
            self.mp.delenv(k, raising=False)


# ---- the matrix, shared by every case ---------------------------------------------------------------------------------------------
def coeff_table(c):
    """every class of coefficient: dropped, +-1, +-2, short and long general values of both signs, the recoding's corners, 20 random"""
    r = c.r
    rng = pyref.Xoshiro(0xC0EF + c.cid)
    return [0, 1, 2, r - 1, r - 2, 3, 8, 9, 1 << 16, r - (1 << 16), 1 << 200, r - 3, (r - 1) // 2, (r + 1) // 2, 0xF << 248] + [
        rng.field(r - 1) + 1 for _ in range(20)]


def magnitude(c, k):
    k %= c.r
    return min(k, c.r - k)


def csr(rows):
    """rows: list of lists of (cid, col) -> (row_start, terms)"""
    row_start = np.zeros(len(rows) + 1, np.uint64)
    row_start[1:] = np.cumsum([len(x) for x in rows])
    terms = np.array([t for x in rows for t in x], dtype=np.uint32).reshape(-1, 2)
    return row_start, terms


def row_logs(c, a, table, rows):
    return [sum(table[cid] * a[col] for cid, col in row) % c.r for row in rows]


def expect_rows(c, group, a, table, rows):
    return fb.expected_points(c, group, row_logs(c, a, table, rows))


def coeff_arr(c, table, mont=False):
    if mont:
        return fr_to_arr(c, [k % c.r for k in table], mont=True)
    return np.array([[(k >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for k in table], dtype=np.uint64)   # (a value >= r stays as it is)


_MATRICES = {}


def class_matrix(c, n_rows):
    """row lengths from {0, 1, 2, 3, 5}, distinct columns inside a row, coefficient ids over the whole table; every id is used at
    n_rows = 1000"""
    if (c.cid, n_rows) not in _MATRICES:
        rng = pyref.Xoshiro(0x3A7 + 31 * n_rows + c.cid)
        ncoef = len(coeff_table(c))
        rows = []
        for _ in range(n_rows):
            cols = []
            while len(cols) < (0, 1, 2, 3, 5)[rng.next() % 5]:
                j = rng.next() % NPTS
                if j not in cols:
                    cols.append(j)
            rows.append([(rng.next() % ncoef, j) for j in cols])
        _MATRICES[(c.cid, n_rows)] = rows
    return _MATRICES[(c.cid, n_rows)]


def run(ctx, c, group, P, rows, table, **kw):
    row_start, terms = csr(rows)
    mont = kw.pop("montgomery", False)
    return ecc.SparsePointSums(ctx, c.name, group, P, row_start, terms, coeff_arr(c, table, mont), montgomery=mont, **kw)


def check(got, want, what=None):
    assert got.shape == want.shape
    bad = np.where((got != want).any(axis=1))[0]
    assert bad.size == 0, (what, bad[:8])


# ---- 1. coefficient classes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "montgomery"])
@pytest.mark.parametrize("c,group", PAIRS, ids=PAIR_IDS)
def test_sparse_sums_coefficient_classes(emu_ctx, c, group, mont, sizes=None):
    """257 points, n_rows in {1, 2, 63, 64, 65, 257, 1000}, every coefficient class, canonical and Montgomery.  redone == 0: the rows have distinct columns, and the digit model of
    tests/test_scale_points.py confirms on the CPU that no magnitude of the table meets an exceptional addition in the ladder"""
    sizes = SIZES if sizes is None else sizes
    table, a, P = coeff_table(c), sp.logs(c, NPTS), sp.points(c, group, NPTS)
    assert not any(sp.hits_exception(magnitude(c, k), c.r) for k in table if magnitude(c, k) > 2)
    for n_rows in sizes:
        rows = class_matrix(c, n_rows)
        if n_rows == 1000:
            assert {cid for row in rows for cid, _ in row} == set(range(len(table)))
        got, redone = run(emu_ctx, c, group, P, rows, table, montgomery=mont)
        check(got, expect_rows(c, group, a, table, rows), (n_rows, mont))
        assert redone == 0, (n_rows, mont, redone)


# ---- 2. row lengths ---------------------------------------------------------------------------------------------------------------------
EDGE_LENGTHS = (0, 1, 3, 4, 5, 15, 16, 17, 64, 65, 257, 0)   # S = 4: 0, 1, S, S + 1, S^2, S^2 + 1 among them; the first and the last row empty


@pytest.mark.parametrize("c,group", PAIRS, ids=PAIR_IDS)
def test_sparse_sums_row_lengths(emu_ctx, monkeypatch, c, group):
    """GA_SPARSE_SEGMENT=4: rows of 0 .. 257 terms are one to five levels of partial sums (4^4 = 256 < 257; the default size needs two from 17 terms on), mixed coefficient
    classes, columns drawn with repetition; the bytes of the default segment size, both orders of the products"""
    table, a, P = coeff_table(c), sp.logs(c, NPTS), sp.points(c, group, NPTS)
    rng = pyref.Xoshiro(0x10E + c.cid)
    rows = [[(rng.next() % len(table), rng.next() % NPTS) for _ in range(n)] for n in EDGE_LENGTHS]
    want = expect_rows(c, group, a, table, rows)
    base, _ = run(emu_ctx, c, group, P, rows, table)
    check(base, want, "default")
    for segment, order in ((4, None), (4, 1), (None, 1)):
        with knobs(monkeypatch, segment=segment, order=order):
            got, _ = run(emu_ctx, c, group, P, rows, table)
        check(got, base, (segment, order))


@pytest.mark.parametrize("c,group", PAIRS, ids=PAIR_IDS)
def test_sparse_sums_long_row(emu_ctx, c, group, length=70000, n_points=1000):
    """default knobs: one row of 70 000 terms with coefficient 1 over 1 000 points (the constant wire of a circuit) among 100 short
    rows.  redone is not asserted: a segment that starts with a repeated column is a legitimate doubling"""
    table, a, P = coeff_table(c), sp.logs(c, n_points), sp.points(c, group, n_points)
    rng = pyref.Xoshiro(0x70000 + c.cid)
    short = class_matrix(c, 100)
    rows = short[:37] + [[(1, rng.next() % n_points) for _ in range(length)]] + short[37:]
    got, _ = run(emu_ctx, c, group, P, rows, table)
    check(got, expect_rows(c, group, a, table, rows))


# ---- 3. exceptions ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,group", PAIRS, ids=PAIR_IDS)
def test_sparse_sums_exceptions(emu_ctx, monkeypatch, c, group):
    """doublings, cancellations, dropped rows, a point at infinity, a coefficient equal to r, equal and opposite partial sums: every
    result exact, redone > 0 where an addition had to be exceptional and 0 where none was"""
    r = c.r
    a = sp.logs(c, NPTS)
    P = sp.points(c, group, NPTS).copy()
    P[7] = 0
    al = list(a)
    al[7] = 0
    g = coeff_table(c)[20]   # a random full-width value
    cancel = (-g * a[11] * pow(a[12], -1, r)) % r
    table = [0, 1, 2, r - 1, r - 2, g, cancel, r, 3, r - 3, r - g]   # table[7] = r: canonical words that are not below r
    ZERO, ONE, TWO, M1, M2, GEN, CAN, RR, T3, M3, NGEN = range(11)
    zero = fb.expected_points(c, group, [0])[0]
    assert not zero.any()

    def one(rows, **kw):
        got, redone = run(emu_ctx, c, group, P, rows, table, **kw)
        check(got, expect_rows(c, group, al, table, rows), rows[:2])
        return got, redone

    got, redone = one([[(ONE, 3), (ONE, 3)]])                      # {+P3, +P3} -> 2 P3
    assert redone >= 1 and got.any()
    for row in ([(ONE, 3), (M1, 3)], [(TWO, 3), (M1, 3), (M1, 3)], [(GEN, 11), (CAN, 12)]):
        got, redone = one([row])                                   # -> (0,0), through the complete formulas
        assert redone >= 1 and not got.any()
    quiet = [[(ZERO, 1), (ZERO, 2), (ZERO, 3)],                    # every coefficient 0
             [(T3, 7), (ONE, 7), (M2, 7), (ONE, 5), (GEN, 9)],     # a (0,0) point under non-zero coefficients, among other terms
             [(RR, 4), (ONE, 6)], [(RR, 4)],                       # r itself behaves as 0
             [(ONE, 7)], []]
    got, redone = one(quiet)
    assert redone == 0 and not got[0].any() and not got[3].any() and not got[4].any() and not got[5].any()
    first = [(GEN, 21), (ONE, 22), (M2, 23), (T3, 24)]
    opposite = [(NGEN, 21), (M1, 22), (TWO, 23), (M3, 24)]
    with knobs(monkeypatch, segment=4):
        got, redone = one([first + first, [(ONE, 30)], first + opposite])
    assert redone >= 2 and got[0].any() and not got[2].any()
    everything = [[(ONE, 3), (ONE, 3)], [(ONE, 3), (M1, 3)], [(TWO, 3), (M1, 3), (M1, 3)], [(GEN, 11), (CAN, 12)]] + quiet
    got, redone = one(everything)
    assert redone >= 4


# ---- 4. chunks --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,group", PAIRS, ids=PAIR_IDS)
def test_sparse_sums_chunks(emu_ctx, monkeypatch, c, group):
    """300 general terms in passes of 64 (GA_SPARSE_CHUNK; four whole passes and one of 44) give the bytes of one pass, in row order
    and in coefficient order"""
    table, a, P = coeff_table(c), sp.logs(c, NPTS), sp.points(c, group, NPTS)
    rng = pyref.Xoshiro(0xC4C + c.cid)
    general = [i for i, k in enumerate(table) if magnitude(c, k) > 2]
    rows = [[(general[rng.next() % len(general)], (7 * i + 85 * j) % NPTS) for j in range(3)] for i in range(100)]   # distinct columns in a row
    want = expect_rows(c, group, a, table, rows)
    base, redone = run(emu_ctx, c, group, P, rows, table)
    check(base, want)
    assert redone == 0
    for order in (None, 1):
        with knobs(monkeypatch, chunk=64, order=order):
            got, redone = run(emu_ctx, c, group, P, rows, table)
        check(got, base, order)
        assert redone == 0


# ---- 5. placement and purity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,group", PAIRS, ids=PAIR_IDS)
def test_sparse_sums_placement_and_purity(emu_ctx, c, group, n_rows=64):
    """host / device points x host / device output: equal bytes; the inputs are byte-identical afterwards; a second call gives the
    same bytes; GA_RESULT_BITREVERSED is the natural result permuted"""
    ctx, wa = emu_ctx, affine_words(c.cid, group)
    table, a, P = coeff_table(c), sp.logs(c, NPTS), sp.points(c, group, NPTS)
    rows = class_matrix(c, n_rows)
    row_start, terms = csr(rows)
    co = coeff_arr(c, table)
    want = expect_rows(c, group, a, table, rows)
    keep = [x.copy() for x in (P, row_start, terms, co)]
    d_in = ctx.to_device(P)
    try:
        for pts in (P, d_in):
            for _ in range(2):
                got, _ = ecc.SparsePointSums(ctx, c.name, group, pts, row_start, terms, co, n_points=NPTS)
                check(got, want)
            d_out, _ = ecc.SparsePointSums(ctx, c.name, group, pts, row_start, terms, co, n_points=NPTS, out_device=True)
            try:
                check(d_out.to_host((n_rows, wa)), want)
            finally:
                d_out.free()
            rev, _ = ecc.SparsePointSums(ctx, c.name, group, pts, row_start, terms, co, n_points=NPTS, bitreversed=True)
            check(rev[[pyref.bitrev(i, 6) for i in range(n_rows)]], want, "bitreversed")
        assert all(np.array_equal(x, y) for x, y in zip((P, row_start, terms, co), keep))
        assert np.array_equal(d_in.to_host((NPTS, wa)), keep[0])
    finally:
        d_in.free()


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_sparse_sums_errors(emu_ctx, monkeypatch, c, n_rows=6):
    """every GA_ERR_INVALID of include/gnark_amd.h with its message, nothing written, each followed by a valid call on the same
    context; n_rows = 0; the binding's own length check; GA_FAULT_THROW"""
    ctx, lib, h = emu_ctx, emu_ctx.lib, emu_ctx.handle
    wa = affine_words(c.cid, 0)
    table, a, P = coeff_table(c), sp.logs(c, NPTS), sp.points(c, 0, NPTS)
    rows = class_matrix(c, 65)[30:30 + n_rows]
    assert sum(len(x) for x in rows) >= 4
    row_start, terms = csr(rows)
    co = coeff_arr(c, table)
    want = expect_rows(c, 0, a, table, rows)
    out = np.full((8, wa), 0xAB, np.uint64)
    red = C.c_uint64(77)
    p = lambda x: x.ctypes.data

    def call(handle=h, curve=c.cid, group=0, points=p(P), n_points=NPTS, rs=row_start, nr=n_rows, tm=terms, coeffs=p(co), nc=len(table), flags=0, o=p(out)):
        return lib.ga_sparse_point_sums(handle, curve, group, points, n_points, None if rs is None else p(rs), nr, None if tm is None else p(tm), coeffs, nc, flags,
                                        o, C.byref(red))

    down, shifted, short_end = row_start.copy(), row_start.copy(), row_start.copy()
    k = next(i for i in range(1, n_rows) if row_start[i + 1] > row_start[i] > 0)
    down[k] = row_start[k + 1] + 1                       # row k - 1 ends after row k does
    shifted[0] = 1
    assert row_start[n_rows - 1] >= 1
    short_end[n_rows] = row_start[n_rows - 1] - 1        # fewer terms than the rows before the last one hold
    big_cid, big_col = terms.copy(), terms.copy()
    big_cid[2, 0] = len(table)
    big_col[1, 1] = NPTS
    bad = [
        (dict(curve=7), "unknown curve"), (dict(group=2), "group id"),
        (dict(handle=None), "null"), (dict(points=None), "null"), (dict(rs=None), "null"), (dict(tm=None), "null"), (dict(coeffs=None), "null"),
        (dict(o=None), "null"),
        (dict(rs=down), "row_start decreases"), (dict(rs=shifted), "row_start[0]"), (dict(rs=short_end), "row_start decreases"),
        (dict(tm=big_cid), "cid %d" % len(table)), (dict(tm=big_col), "col %d" % NPTS),
        (dict(nc=int(terms[:, 0].max())), "coefficients"), (dict(n_points=int(terms[:, 1].max())), "points"),
        (dict(flags=_lib.RESULT_BITREVERSED), "power-of-two"),
    ]
    for kw, message in bad:
        assert call(**kw) == -1, kw
        assert message in lib.ga_last_error().decode(), (kw, lib.ga_last_error())
        assert (out == 0xAB).all()
        got, redone = ecc.SparsePointSums(ctx, c.name, 0, P, row_start, terms, co)
        check(got, want)
    with pytest.raises(ValueError, match="row_start"):       # the C signature carries no nnz: row_start[n_rows] IS the number of terms
        ecc.SparsePointSums(ctx, c.name, 0, P, row_start, terms[:-1], co)
    with pytest.raises(GnarkAmdError, match="power-of-two"):
        ecc.SparsePointSums(ctx, c.name, 0, P, row_start, terms, co, bitreversed=True)
    assert call(nr=0) == 0 and red.value == 0 and (out == 0xAB).all()
    assert lib.ga_sparse_point_sums(h, c.cid, 0, None, 0, None, 0, None, None, 0, 0, None, None) == 0
    got, redone = ecc.SparsePointSums(ctx, c.name, 0, P, np.zeros(1, np.uint64), np.zeros((0, 2), np.uint32), co)
    assert got.shape == (0, wa) and redone == 0
    empty = np.zeros(4, np.uint64)                            # three empty rows: no terms, so no points and no coefficients either
    assert lib.ga_sparse_point_sums(h, c.cid, 0, None, 0, p(empty), 3, None, None, 0, 0, p(out), None) == 0 and not out[:3].any() and (out[3:] == 0xAB).all()
    try:
        monkeypatch.setenv("GA_FAULT_THROW", "ga_sparse_point_sums")
        with pytest.raises(GnarkAmdError, match=r"error -3: out of host memory \(std::bad_alloc\) under ga_sparse_point_sums"):
            ecc.SparsePointSums(ctx, c.name, 0, P, row_start, terms, co)
        monkeypatch.delenv("GA_FAULT_THROW")
        got, _ = ecc.SparsePointSums(ctx, c.name, 0, P, row_start, terms, co)
        check(got, want)
    finally:
        monkeypatch.delenv("GA_FAULT_THROW", raising=False)


# ---- the transform ------------------------------------------------------------------------------------------------------------------------
LAGRANGE_SIZES = (1, 2, 4, 8, 64, 128, 256)


@pytest.mark.parametrize("uniform", [1, 0], ids=["uniform", "consecutive"])
@pytest.mark.parametrize("c,group", PAIRS, ids=PAIR_IDS)
def test_lagrange_coeffs_known_tau(emu_ctx, monkeypatch, c, group, uniform, sizes=None):
    """powers = [tau^i]G -> [l_i(tau)]G in G1 and in G2, both lane orders (n = 1024 where the emulation affords it: G1)"""
    if sizes is None:
        sizes = LAGRANGE_SIZES + ((1024,) if group == 0 and uniform else ())
    tau = tl.tau_of(c)
    for n in sizes:
        powers = fb.expected_points(c, group, tl.powers_of(c, n, tau))
        want = fb.expected_points(c, group, tl.lagrange_scalars(c, n, tau))
        with knobs(monkeypatch, uniform=uniform):
            got = ecc.LagrangeCoeffs(emu_ctx, c.name, group, powers)
        check(got, want, n)


@pytest.mark.parametrize("n", [16, 64, 256])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_lagrange_coeffs_degenerate_g2(emu_ctx, c, n):
    """the two inputs of test_to_lagrange_degenerate in G2: all inputs the same point -> out[0] = P, (0,0) elsewhere; tau = w ->
    out[1] = G, (0,0) elsewhere"""
    wa = affine_words(c.cid, 1)
    P = fb.expected_points(c, 1, [0xC0FFEE])
    want = np.zeros((n, wa), np.uint64)
    want[0] = P[0]
    check(ecc.LagrangeCoeffs(emu_ctx, c.name, 1, np.repeat(P, n, axis=0)), want)
    powers = fb.expected_points(c, 1, tl.powers_of(c, n, c.fr_root_of_unity(n)))
    want = np.zeros((n, wa), np.uint64)
    want[1] = fb.gen_arr(c, 1)[0]
    check(ecc.LagrangeCoeffs(emu_ctx, c.name, 1, powers), want)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_lagrange_coeffs_random_g2_points_with_infinities(emu_ctx, c, n=32):
    """32 unrelated G2 points, three of them (0,0), against out[i] = [1/n] sum_j [w^(-ij)] in[j] row by row with oracle.msm"""
    rng = pyref.Xoshiro(0x1A62 + c.cid)
    P = oracle.gen_bases(c.cid, 1, np.array([rng.next() for _ in range(n)], dtype=np.uint64)).copy()
    for j in (0, 13, 31):
        P[j] = 0
    winv, ninv = pow(c.fr_root_of_unity(n), -1, c.r), pow(n, -1, c.r)
    want = np.stack([oracle.jac_to_affine(c.cid, 1, oracle.msm(c.cid, 1, P, fr_to_arr(c, [pow(winv, i * j, c.r) * ninv % c.r for j in range(n)])))
                     for i in range(n)])
    check(ecc.LagrangeCoeffs(emu_ctx, c.name, 1, P), want)


def test_lagrange_coeffs_g1_is_to_lagrange_g1(emu_ctx, n=256):
    """group = GA_G1 returns the bytes of ga_kzg_to_lagrange_g1 on the EIP-4844 ceremony SRS (its first n points: any n points of the
    group are a valid input), host and device"""
    mono, _ = tl.golden_srs()
    mono = mono[:n].copy()
    want = ecc.ToLagrangeG1(emu_ctx, BLS12_381.name, mono)
    assert want.any(axis=1).all()
    check(ecc.LagrangeCoeffs(emu_ctx, BLS12_381.name, 0, mono), want)
    d_in = emu_ctx.to_device(mono)
    try:
        d_out = ecc.LagrangeCoeffs(emu_ctx, BLS12_381.name, 0, d_in, n=n, out_device=True)
        try:
            check(d_out.to_host(want.shape), want)
        finally:
            d_out.free()
    finally:
        d_in.free()


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_lagrange_coeffs_errors(emu_ctx, c, n=16):
    """n not a power of two, n above the two-adicity of r, an unknown group or curve, null pointers: GA_ERR_INVALID with the entry
    point's name, nothing written, and the next valid call succeeds; n = 0 is GA_OK"""
    ctx, lib, h = emu_ctx, emu_ctx.lib, emu_ctx.handle
    wa = affine_words(c.cid, 1)
    tau = tl.tau_of(c)
    powers = fb.expected_points(c, 1, tl.powers_of(c, n, tau))
    want = fb.expected_points(c, 1, tl.lagrange_scalars(c, n, tau))
    out = np.full((n, wa), 0xAB, np.uint64)
    p = lambda x: x.ctypes.data
    for args in ((h, c.cid, 1, p(powers), 3, 0, p(out)), (h, c.cid, 1, p(powers), 12, 0, p(out)),
                 (h, c.cid, 1, p(powers), 1 << (tl.ADICITY[c.name] + 1), 0, p(out)),
                 (h, c.cid, 2, p(powers), n, 0, p(out)), (h, c.cid, -1, p(powers), n, 0, p(out)), (h, 7, 1, p(powers), n, 0, p(out)),
                 (h, c.cid, 1, None, n, 0, p(out)), (h, c.cid, 1, p(powers), n, 0, None), (None, c.cid, 1, p(powers), n, 0, p(out))):
        assert lib.ga_lagrange_coeffs(*args) == -1, args[1:6]
        assert "ga_lagrange_coeffs" in lib.ga_last_error().decode()
        assert (out == 0xAB).all()
        check(ecc.LagrangeCoeffs(ctx, c.name, 1, powers), want)
    assert lib.ga_lagrange_coeffs(h, c.cid, 1, None, 0, 0, None) == 0
    with pytest.raises(GnarkAmdError, match="power of two"):
        ecc.LagrangeCoeffs(ctx, c.name, 1, powers[:12])


# ---- Phase2.Initialize, replayed ----------------------------------------------------------------------------------------------------------
def random_r1cs(c, n_constraints, n_wires, seed):
    """a seeded R1CS with the coefficient mix of coeff_table, wire 0 in many constraints, some wires missing from L or R"""
    rng = pyref.Xoshiro(seed + c.cid)
    table = coeff_table(c)

    def lin(lo):
        row = {}
        for _ in range(1 + rng.next() % 3):
            row[lo + rng.next() % (n_wires - lo)] = table[rng.next() % len(table)]
        if rng.next() % 2:
            row[0] = table[rng.next() % len(table)]
        return row
    return pyref.R1CS(nb_public=2, nb_wires=n_wires, L=[lin(n_wires // 4) for _ in range(n_constraints)], R=[lin(n_wires // 3) for _ in range(n_constraints)],
                      O=[lin(1) for _ in range(n_constraints)])


def setup_scalars(c, cs, alpha, beta, tau):
    """the discrete logs of Initialize's vectors (pyref.groth16_setup's, with gamma = delta = 1, without its point arithmetic)"""
    mod, m = c.r, len(cs.L)
    n = 1
    while n < m:
        n *= 2
    lag = tl.lagrange_scalars(c, n, tau)
    Av, Bv, Cv = [0] * cs.nb_wires, [0] * cs.nb_wires, [0] * cs.nb_wires
    for M, V in ((cs.L, Av), (cs.R, Bv), (cs.O, Cv)):
        for i in range(m):
            for wi, k in M[i].items():
                V[wi] = (V[wi] + k * lag[i]) % mod
    kk = [(beta * x + alpha * y + z) % mod for x, y, z in zip(Av, Bv, Cv)]
    tn1 = (pow(tau, n, mod) - 1) % mod
    Z = pyref.bitrev_permute([pow(tau, i, mod) * tn1 % mod for i in range(n)])[:n - 1]
    return n, dict(A=Av, B=Bv, K=kk, Z=Z)


def wire_major(cs, n):
    """gnark's constraint-major matrices -> the wire-major CSR rows ga_sparse_point_sums takes (a counting sort on the host), with one
    coefficient table for all of them: rows of L, of R, and of [L | R | O] over the concatenation with column offsets 0, n, 2n"""
    values = sorted({k for M in (cs.L, cs.R, cs.O) for row in M for k in row.values()})
    cid = {k: i for i, k in enumerate(values)}

    def transpose(blocks):
        rows = [[] for _ in range(cs.nb_wires)]
        for off, M in blocks:
            for i, row in enumerate(M):
                for wi, k in row.items():
                    rows[wi].append((cid[k], off + i))
        return rows
    return values, transpose([(0, cs.L)]), transpose([(0, cs.R)]), transpose([(0, cs.L), (n, cs.R), (2 * n, cs.O)])


def phase2_initialize(ctx, c, cs, alpha, beta, tau):
    """Initialize as INTEGRATION.md maps it: the commons with BatchScalarMultiplication, four LagrangeCoeffs, five SparsePointSums;
    nothing but the matrices goes through the host.  Returns device buffers A, B, B2, K (one point per wire) and Z (n points, the last
    one (0,0)), and n; the caller frees them"""
    lib, h = ctx.lib, ctx.handle
    m = len(cs.L)
    n = 1
    while n < m:
        n *= 2
    w1, w2 = affine_words(c.cid, 0) * 8, affine_words(c.cid, 1) * 8
    pw = tl.powers_of(c, 2 * n - 1, tau)
    bufs, out = {}, {}
    try:
        commons = {"tau1": (0, 1, 2 * n - 1), "tau2": (1, 1, n), "alpha": (0, alpha, n), "beta": (0, beta, n)}
        for k, (g, f, cnt) in commons.items():
            bufs[k] = ecc.BatchScalarMultiplication(ctx, c.name, g, fb.gen_arr(c, g), fb.canon(c, [f * x % c.r for x in pw[:cnt]]), out_device=True)
        # the three G1 transforms land side by side: [BetaTau | AlphaTau | Tau] in Lagrange form is the point vector of K
        bufs["cat"] = ctx.malloc(3 * n * w1)
        flags = _lib.BASES_ON_DEVICE | _lib.RESULT_ON_DEVICE
        for j, k in enumerate(("beta", "alpha", "tau1")):
            lib.check(lib.ga_lagrange_coeffs(h, c.cid, 0, C.c_void_p(bufs[k].ptr), n, flags, C.c_void_p(bufs["cat"].offset(j * n * w1))))
        bufs["lag2"] = ecc.LagrangeCoeffs(ctx, c.name, 1, bufs["tau2"], n=n, out_device=True)
        values, rows_l, rows_r, rows_k = wire_major(cs, n)
        co = coeff_arr(c, values)
        lag_tau = bufs["cat"].offset(2 * n * w1)
        for name, g, pts, npts, rows in (("A", 0, lag_tau, n, rows_l), ("B", 0, lag_tau, n, rows_r), ("B2", 1, bufs["lag2"], n, rows_r),
                                         ("K", 0, bufs["cat"], 3 * n, rows_k)):
            row_start, terms = csr(rows)
            out[name], _ = ecc.SparsePointSums(ctx, c.name, g, pts, row_start, terms, co, n_points=npts, out_device=True)
        zrows = [[(0, i + n), (1, i)] for i in range(n - 1)] + [[]]   # Z[i] = Tau[i + n] - Tau[i]; row n - 1 would need Tau[2n - 1]
        row_start, terms = csr(zrows)
        out["Z"], _ = ecc.SparsePointSums(ctx, c.name, 0, bufs["tau1"], row_start, terms, coeff_arr(c, [1, c.r - 1]), n_points=2 * n - 1,
                                          bitreversed=True, out_device=True)
        return out, n
    except Exception:
        for b in out.values():
            b.free()
        raise
    finally:
        for b in bufs.values():
            b.free()


CIRCUITS = {"cubic": lambda c: pyref.cubic_r1cs(), "commit": lambda c: pyref.commit_r1cs(), "random": lambda c: random_r1cs(c, 60, 40, 0x60C5)}


@pytest.mark.parametrize("circuit", list(CIRCUITS))
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_phase2_initialize_replay(emu_ctx, c, circuit):
    """every vector of Initialize against pyref.groth16_setup(c, cs, (alpha, beta, 1, 1, tau)) -- gamma = delta = 1 is exactly
    Initialize's state: A, B, B2 unfiltered ((0,0) where infinityA / infinityB say so), K for all wires against dlog["kk"], Z
    bit-reversed, n - 1 points"""
    from helpers import pts_to_arr
    cs = CIRCUITS[circuit](c)
    rng = pyref.Xoshiro(0x1417 + c.cid)
    alpha, beta, tau = (rng.field(c.r - 1) + 1 for _ in range(3))
    toxic = [alpha, beta, 1, 1, tau] + [1] * (len(cs.commitments) + 1)
    pk, _, dlog = pyref.groth16_setup(c, cs, toxic)
    n, logs = setup_scalars(c, cs, alpha, beta, tau)
    assert n == pk.n and logs["K"] == dlog["kk"] and logs["Z"] == dlog["Z"] and [x for x in logs["A"] if x] == dlog["A"]
    if circuit == "random":
        assert n == 64 and any(pk.infinityA) and any(pk.infinityB)

    def unfiltered(group, pts, inf):
        full = np.zeros((cs.nb_wires, affine_words(c.cid, group)), np.uint64)
        full[[i for i, z in enumerate(inf) if not z]] = pts_to_arr(c, group, pts)
        return full
    want = {"A": unfiltered(0, pk.A, pk.infinityA), "B": unfiltered(0, pk.B, pk.infinityB), "B2": unfiltered(1, pk.B2, pk.infinityB),
            "K": fb.expected_points(c, 0, dlog["kk"]), "Z": pts_to_arr(c, 0, pk.Z)}
    out, n = phase2_initialize(emu_ctx, c, cs, alpha, beta, tau)
    try:
        for k, w in want.items():
            got = out[k].to_host((n if k == "Z" else cs.nb_wires, w.shape[1]))
            if k == "Z":
                assert not got[n - 1].any()
                got = got[:n - 1]
            check(got, w, k)
    finally:
        for b in out.values():
            b.free()


# ---- bindings and bounds ------------------------------------------------------------------------------------------------------------------
def test_phase2_symbols_and_go_bindings(emu_lib):
    """both entry points are exported and bound; ga.go calls them and go/IDENTS.json resolves the calls against the header"""
    header = open(os.path.join(ROOT, "include", "gnark_amd.h")).read()
    assert "int ga_lagrange_coeffs(ga_ctx* ctx, int curve, int group, const void* powers_affine, size_t n, unsigned flags, void* out_affine);" in header
    assert "int ga_sparse_point_sums(ga_ctx* ctx, int curve, int group, const void* points_affine, size_t n_points," in header
    go = open(os.path.join(ROOT, "go", "backend", "accelerated", "mi355x", "internal", "ga", "ga.go")).read()
    idents = json.load(open(os.path.join(ROOT, "go", "IDENTS.json")))["resolved"]
    for name, func, nargs in (("ga_lagrange_coeffs", "LagrangeCoeffs", 7), ("ga_sparse_point_sums", "SparsePointSums", 13)):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(emu_lib, name)
        assert f"func (c *Context) {func}(" in go and f"C.{name}(c.h, C.int(curve), C.int(group)," in go
        assert ["go/backend/accelerated/mi355x/internal/ga/ga.go", f"C.{name}", f"include/gnark_amd.h prototype ({nargs} args)"] in idents


@pytest.mark.parametrize("fp2", [False, True], ids=["G1", "G2"])
@pytest.mark.parametrize("curve", ["bn254", "bls12-381"])
def test_sparse_sums_bounds(curve, fp2):
    """the row-sum kernel is made of add29, dbl29 and the negation of a canonical y only -- the closed set that
    tools/lazy_bounds.py check_ladder(curve, fp2) bounds; the negation comes BEFORE the doubling (dbl29's y is not canonical)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import lazy_bounds
    out = lazy_bounds.check_ladder(curve, fp2)
    assert all(v < out["limit"] - 2.5 for k, v in out.items() if k != "limit")
    src = open(os.path.join(ROOT, "gnark_amd", "csrc", "sparse_sums.hip.h")).read()
    body = src[src.index("bool sparse_operand("):src.index("// the flagged segments of a level")]
    assert body.count("add29<F>(") == 1 and body.count("dbl29<F>(") == 1
    assert body.count("f29_sub<2>(") == 1 and "f29_sub<" not in body.replace("f29_sub<2>(", "") and "f29_mul" not in body and "f29_add" not in body
    assert body.index("f29_sub<2>(") < body.index("dbl29<F>(")

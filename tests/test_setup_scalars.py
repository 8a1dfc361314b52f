"""The scalar side of groth16.Setup on the device (backend/groth16/<curve>/setup.go:142-219,346-428): ga_fr_lagrange_at,
ga_fr_sparse_matvec, ga_fr_compact_nonzero, ga_fr_powers (gnark_amd/csrc/fr_sparse.hip.h, fr_setup.hip.h) and g16_setup.Setup on the
functional emulation.  Every case is a function of a context; tests/test_setup_scalars_gpu.py runs the same cases on the device.
Expected values are Python integers mod r; every comparison is equality of words."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import pyref
import test_fixed_base as fb
import test_phase2_init as cases
import test_to_lagrange as tl
from gnark_amd import _lib, g16_setup
from gnark_amd._lib import GnarkAmdError
from gnark_amd.device import affine_words
from helpers import BLS12_381, BN254, arr_to_fr, fr_to_arr, pts_to_arr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = [BN254, BLS12_381]
FORMS = [False, True]
FORM_IDS = ["canonical", "montgomery"]
NX = 257


class segment:
    """GA_FR_SPARSE_SEGMENT for the calls inside the block (read once per entry point)"""

    def __init__(self, monkeypatch, s):
        self.mp, self.s = monkeypatch, s

    def __enter__(self):
        if self.s is None:
            self.mp.delenv("GA_FR_SPARSE_SEGMENT", raising=False)
        else:
            self.mp.setenv("GA_FR_SPARSE_SEGMENT", str(self.s))

    def __exit__(self, *a):
        self.mp.delenv("GA_FR_SPARSE_SEGMENT", raising=False)


def words(c, ks, mont):
    """ints -> elements in the form of the call; a canonical value that is not below r stays as it is"""
    return cases.coeff_arr(c, ks, mont)


def ints(c, arr, mont):
    return arr_to_fr(c, arr, mont=mont)


_X = {}


def x_values(c, n=NX):
    if (c.cid, n) not in _X:
        rng = pyref.Xoshiro(0x5E7 + c.cid + n)
        _X[(c.cid, n)] = [rng.field(c.r) for _ in range(n)]
    return _X[(c.cid, n)]


def matvec_want(c, x, table, rows, scales=None, row_class=None):
    out = cases.row_logs(c, x, table, rows)
    if scales is not None:
        out = [v * scales[k] % c.r for v, k in zip(out, row_class)]
    return out


def matvec(ctx, c, x, rows, table, mont, **kw):
    row_start, terms = cases.csr(rows)
    if "row_scales" in kw:
        kw["row_scales"] = words(c, kw["row_scales"], mont)
    if not isinstance(x, g16_setup.DeviceBuffer):
        x = words(c, x, mont)
    return g16_setup.SparseMatVec(ctx, c.name, x, row_start, terms, words(c, table, mont), montgomery=mont, **kw)


# ---- 1. Lagrange ------------------------------------------------------------------------------------------------------------------------
def lagrange_want(c, n, tau, m):
    """tl.lagrange_scalars, and zeros for tau inside the domain (tau^n = 1), where fr.BatchInvert leaves inv(0) = 0"""
    if pow(tau, n, c.r) == 1:
        return [0] * m
    return tl.lagrange_scalars(c, n, tau)[:m]


def lagrange_taus(c, n):
    taus = [tl.tau_of(c), 0, 1, c.r - 1]
    if n == 64:
        taus.append(pow(c.fr_root_of_unity(64), 3, c.r))
    return taus


@pytest.mark.parametrize("mont", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_lagrange_at(emu_ctx, c, mont, sizes=(1, 2, 4, 64, 1024)):
    """n in {1, 2, 4, 64, 1024}, m in {n, n - 1, 1}; tau random, 0, 1 = w^0, r - 1 (= w^(n/2) from n = 2 on), w^3 for n = 64"""
    for n in sizes:
        for tau in lagrange_taus(c, n):
            full = lagrange_want(c, n, tau, n)
            if pow(tau, n, c.r) == 1:
                assert not any(full)
            for m in sorted({n, n - 1, 1}):
                got = g16_setup.LagrangeAt(emu_ctx, c.name, n, words(c, [tau], mont)[0], m, montgomery=mont)
                assert got.shape == (m, 4)
                assert ints(c, got, mont) == full[:m], (n, m, tau)


# ---- 2. matvec, the coefficient table -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mont", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_matvec_coefficient_table(emu_ctx, c, mont):
    """class_matrix over 257 random x for n_rows in {1, 2, 63, 64, 65, 257, 1000}, plus one row over three more coefficients: r, r + 7
    and 2^256 - 1 -- canonical words that are not below r (Montgomery: their residues); so is the canonical x[5] (x[5] + r)"""
    base, x = cases.coeff_table(c), list(x_values(c))
    table = base + [c.r, c.r + 7, (1 << 256) - 1]
    xin = list(x)
    if not mont:
        assert x[5] + c.r < (1 << 256)
        xin[5] = x[5] + c.r
    for n_rows in fb.SIZES:
        rows = list(cases.class_matrix(c, n_rows)) + [[(len(base), 1), (len(base) + 1, 5), (len(base) + 2, 3), (2, 5)]]
        got = matvec(emu_ctx, c, xin, rows, table, mont)
        assert ints(c, got, mont) == matvec_want(c, x, table, rows), n_rows


# ---- 3. matvec, row lengths and levels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 16])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_matvec_row_lengths(emu_ctx, monkeypatch, c, S):
    """rows of 0, 1, S - 1, S, S + 1, S^2 and S^2 + 1 terms, one of 5 000 terms with repeated columns and an empty last row (the first
    is empty too): the terms and three levels of partial sums at S = 16 (16^3 < 5 000), thirteen launches at S = 2"""
    table, x = cases.coeff_table(c), x_values(c)
    rng = pyref.Xoshiro(0x10E5 + c.cid + S)
    lengths = [0, 1, S - 1, S, S + 1, S * S, S * S + 1, 5000, 0]
    rows = [[(rng.next() % len(table), rng.next() % NX) for _ in range(n)] for n in lengths]
    levels, n = 1, 5000
    while n > S:
        n, levels = (n + S - 1) // S, levels + 1
    assert levels == {2: 13, 16: 4}[S]
    want = matvec_want(c, x, table, rows)
    for mont in FORMS:
        with segment(monkeypatch, S):
            got = matvec(emu_ctx, c, x, rows, table, mont)
        assert ints(c, got, mont) == want, mont


# ---- 4. matvec, row scales ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mont", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_matvec_row_scales(emu_ctx, monkeypatch, c, mont, n_rows=65):
    """three classes with scales {1, 0, random}, every class used, an empty row with the random scale, a long row (two levels) with it;
    null class and scale pointers give the unscaled rows"""
    table, x = cases.coeff_table(c), x_values(c)
    rng = pyref.Xoshiro(0x5CA1E + c.cid)
    scales = [1, 0, rng.field(c.r - 2) + 2]
    rows = list(cases.class_matrix(c, n_rows))
    rows.append([(rng.next() % len(table), rng.next() % NX) for _ in range(40)])
    row_class = [i % 3 for i in range(len(rows))]
    empty = next(i for i, row in enumerate(rows) if not row)
    row_class[empty], row_class[-1] = 2, 2
    assert set(row_class) == {0, 1, 2}
    plain = matvec_want(c, x, table, rows)
    want = matvec_want(c, x, table, rows, scales, row_class)
    assert want[empty] == 0 and want[-1] != plain[-1]
    got = matvec(emu_ctx, c, x, rows, table, mont, row_class=row_class, row_scales=scales)
    assert ints(c, got, mont) == want
    assert ints(c, matvec(emu_ctx, c, x, rows, table, mont), mont) == plain


# ---- 6. compaction --------------------------------------------------------------------------------------------------------------------
def compaction_vector(c, n, density, seed=0):
    """density 0, 100 or 30 (% zeros); at 30 % index 0 and index n - 1 are zero"""
    rng = pyref.Xoshiro(0xC0 + 7 * n + density + seed + c.cid)
    v = [0 if density == 100 or (density == 30 and rng.next() % 10 < 3) else rng.field(c.r - 1) + 1 for _ in range(n)]
    if density == 30 and n:
        v[0] = v[n - 1] = 0
    return v


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_compact_nonzero(emu_ctx, c, sizes=(0, 1, 63, 64, 65, 257, 1000)):
    """n in {0, 1, 63, 64, 65, 257, 1000} x zero densities 0 %, 100 %, about 30 % (zeros at index 0 and n - 1), out of place and in
    place, host and device: the kept elements in order, the mask and the count; what lies past the count is not written"""
    ctx = emu_ctx
    for n in sizes:
        for density in (0, 100, 30):
            v = compaction_vector(c, n, density)
            kept = [k for k in v if k]
            arr = fr_to_arr(c, v)
            keep = arr.copy()
            out, mask, count = g16_setup.CompactNonZero(ctx, c.name, arr)
            assert count == len(kept) and list(mask) == [k == 0 for k in v] and np.array_equal(arr, keep), (n, density)
            assert arr_to_fr(c, out[:count]) == kept and not out[count:].any()
            same, mask, count = g16_setup.CompactNonZero(ctx, c.name, arr, in_place=True)
            assert same is arr and count == len(kept) and list(mask) == [k == 0 for k in v]
            assert np.array_equal(arr[:count], out[:count]) and np.array_equal(arr[count:], keep[count:])
            if n == 0:
                continue
            d_v = ctx.to_device(keep)
            try:
                d_out, mask, count = g16_setup.CompactNonZero(ctx, c.name, d_v, n, out_device=True)
                try:
                    assert count == len(kept) and list(mask) == [k == 0 for k in v]
                    assert np.array_equal(d_out.to_host((n, 4))[:count], out[:count]) and np.array_equal(d_v.to_host((n, 4)), keep)
                finally:
                    d_out.free()
                host, _, count = g16_setup.CompactNonZero(ctx, c.name, d_v, n, mask=False)
                assert np.array_equal(host[:count], out[:count])
                same, mask, count = g16_setup.CompactNonZero(ctx, c.name, d_v, n, in_place=True)
                assert same is d_v and count == len(kept)
                assert np.array_equal(d_v.to_host((n, 4)), arr)
            finally:
                d_v.free()


# ---- 7. powers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mont", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_powers(emu_ctx, c, mont, sizes=(1, 2, 65, 1000)):
    """n in {1, 2, 65, 1000} x first in {0, 7, 2^40} x t in {0, 1, random} x c in {0, random}; 0^0 = 1 as in fr.Element.Exp"""
    rng = pyref.Xoshiro(0x90E5 + c.cid)
    for n in sizes:
        for first in (0, 7, 1 << 40):
            for t in (0, 1, rng.field(c.r - 2) + 2):
                for k in (0, rng.field(c.r - 1) + 1):
                    ct = words(c, [k, t], mont)
                    got = g16_setup.Powers(emu_ctx, c.name, ct[0], ct[1], n, first, montgomery=mont)
                    want, p = [], pow(t, first, c.r)
                    for _ in range(n):
                        want.append(k * p % c.r)
                        p = p * t % c.r
                    assert ints(c, got, mont) == want, (n, first, t, k)


# ---- 8. placement, purity, errors -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_placement_and_purity(emu_ctx, c, n_rows=64):
    """host / device x, host / device out: the same words, for all four calls; the inputs are unchanged afterwards"""
    ctx = emu_ctx
    table, x = cases.coeff_table(c), x_values(c)
    rows = cases.class_matrix(c, n_rows)
    row_start, terms = cases.csr(rows)
    xa, co = fr_to_arr(c, x), words(c, table, True)
    rc, sc = np.array([i % 2 for i in range(n_rows)], np.uint8), fr_to_arr(c, [3, 5])
    want = fr_to_arr(c, matvec_want(c, x, table, rows, [3, 5], list(rc)))
    keep = [a.copy() for a in (xa, row_start, terms, co, rc, sc)]
    d_x = ctx.to_device(xa)
    try:
        for xv in (xa, d_x):
            for _ in range(2):
                assert np.array_equal(g16_setup.SparseMatVec(ctx, c.name, xv, row_start, terms, co, row_class=rc, row_scales=sc, montgomery=True, n_cols=NX), want)
            d_out = g16_setup.SparseMatVec(ctx, c.name, xv, row_start, terms, co, row_class=rc, row_scales=sc, montgomery=True, n_cols=NX, out_device=True)
            try:
                assert np.array_equal(d_out.to_host((n_rows, 4)), want)
            finally:
                d_out.free()
        assert all(np.array_equal(a, b) for a, b in zip((xa, row_start, terms, co, rc, sc), keep))
        assert np.array_equal(d_x.to_host((NX, 4)), keep[0])
    finally:
        d_x.free()
    tau = tl.tau_of(c)
    for mont in FORMS:
        lag = g16_setup.LagrangeAt(ctx, c.name, 64, tau, 61, montgomery=mont)
        d_lag = g16_setup.LagrangeAt(ctx, c.name, 64, tau, 61, montgomery=mont, out_device=True)
        pw = g16_setup.Powers(ctx, c.name, 3, tau, 61, 5, montgomery=mont)
        d_pw = g16_setup.Powers(ctx, c.name, 3, tau, 61, 5, montgomery=mont, out_device=True)
        try:
            assert np.array_equal(d_lag.to_host((61, 4)), lag) and np.array_equal(d_pw.to_host((61, 4)), pw)
        finally:
            d_lag.free()
            d_pw.free()


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_errors(emu_ctx, monkeypatch, c, n_rows=6):
    """every GA_ERR_INVALID of include/gnark_amd.h for the four calls, raised before `out` is written (it keeps its pattern); after each
    error the same context completes a valid call; the n = 0 cases; GA_FAULT_THROW"""
    ctx, lib, h = emu_ctx, emu_ctx.lib, emu_ctx.handle
    table, x = cases.coeff_table(c), x_values(c)
    rows = cases.class_matrix(c, 65)[30:30 + n_rows]
    row_start, terms = cases.csr(rows)
    xa, co = fr_to_arr(c, x, mont=False), words(c, table, False)
    rc, sc = np.array([i % 2 for i in range(n_rows)], np.uint8), fr_to_arr(c, [3, 5], mont=False)
    want = fr_to_arr(c, matvec_want(c, x, table, rows, [3, 5], list(rc)), mont=False)
    out = np.full((64, 4), 0xAB, np.uint64)
    p = lambda a: a.ctypes.data
    tau = fr_to_arr(c, [tl.tau_of(c)], mont=False)
    count = C.c_uint64(99)

    def valid():
        assert np.array_equal(g16_setup.SparseMatVec(ctx, c.name, xa, row_start, terms, co, row_class=rc, row_scales=sc), want)

    def bad(rc_, message):
        assert rc_ == -1, message
        assert message in lib.ga_last_error().decode(), (message, lib.ga_last_error())
        assert (out == 0xAB).all(), message
        valid()

    def mv(handle=h, curve=c.cid, xp=p(xa), n_cols=NX, rs=row_start, nr=n_rows, tm=terms, coeffs=p(co), nc=len(table), cls=rc, scl=sc, ncls=2, o=p(out)):
        return lib.ga_fr_sparse_matvec(handle, curve, xp, n_cols, None if rs is None else p(rs), nr, None if tm is None else p(tm), coeffs, nc,
                                       None if cls is None else p(cls), None if scl is None else p(scl), ncls, 0, o)

    down, shifted, too_many = row_start.copy(), row_start.copy(), row_start.copy()
    too_many[n_rows] = 1 << 32                            # nnz above 2^32 - 1: rejected before any term is read
    k = next(i for i in range(1, n_rows) if row_start[i + 1] > row_start[i] > 0)
    down[k] = row_start[k + 1] + 1
    shifted[0] = 1
    big_cid, big_col, big_class = terms.copy(), terms.copy(), rc.copy()
    big_cid[2, 0] = len(table)
    big_col[1, 1] = NX
    big_class[3] = 2
    for kw, message in [
            (dict(curve=7), "unknown curve"), (dict(handle=None), "null"), (dict(xp=None), "null"), (dict(rs=None), "null"), (dict(tm=None), "null"),
            (dict(coeffs=None), "null"), (dict(o=None), "null"), (dict(cls=None), "come together"), (dict(scl=None), "come together"),
            (dict(ncls=0), "come together"), (dict(ncls=257), "come together"),
            (dict(rs=down), "row_start decreases"), (dict(rs=shifted), "row_start[0]"), (dict(rs=too_many), "at most 2^32 - 1"),
            (dict(tm=big_cid), "cid %d" % len(table)), (dict(tm=big_col), "col %d" % NX),
            (dict(nc=int(terms[:, 0].max())), "coefficients"), (dict(n_cols=int(terms[:, 1].max())), "columns"),
            (dict(cls=big_class), "row_class[3]"), (dict(nr=1 << 31), "n_rows")]:
        bad(mv(**kw), message)
    assert mv(nr=0) == 0 and (out == 0xAB).all()
    empty = np.zeros(4, np.uint64)   # three empty rows: no terms, so no x and no coefficients either
    scratch = out.copy()
    assert lib.ga_fr_sparse_matvec(h, c.cid, None, 0, p(empty), 3, None, None, 0, None, None, 0, 0, p(scratch)) == 0
    assert not scratch[:3].any() and (scratch[3:] == 0xAB).all()
    with pytest.raises(ValueError, match="row_start"):
        g16_setup.SparseMatVec(ctx, c.name, xa, row_start, terms[:-1], co)

    def lag(handle=h, curve=c.cid, n=16, t=p(tau), m=16, o=p(out)):
        return lib.ga_fr_lagrange_at(handle, curve, n, t, m, 0, o)
    for kw, message in [(dict(curve=7), "unknown curve"), (dict(handle=None), "null"), (dict(t=None), "null"), (dict(o=None), "null"),
                        (dict(n=12), "power of two"), (dict(n=0), "power of two"), (dict(n=1 << (tl.ADICITY[c.name] + 1)), "power of two"),
                        (dict(m=17), "above n")]:
        bad(lag(**kw), message)
    assert lag(m=0) == 0 and lag(m=0, t=None, o=None) == 0 and (out == 0xAB).all()

    def compact(handle=h, curve=c.cid, v=p(xa), n=NX // 8, o=p(out), cnt=C.byref(count)):
        return lib.ga_fr_compact_nonzero(handle, curve, v, n, 0, o, None, cnt)
    for kw, message in [(dict(curve=7), "unknown curve"), (dict(handle=None), "null"), (dict(v=None), "null"), (dict(o=None), "null"),
                        (dict(cnt=None), "null count"), (dict(n=1 << 31), "2^31 - 1")]:
        bad(compact(**kw), message)
    assert count.value == 99
    assert compact(n=0, v=None, o=None) == 0 and count.value == 0 and (out == 0xAB).all()

    def powers(handle=h, curve=c.cid, s=p(sc), first=0, n=8, o=p(out)):
        return lib.ga_fr_powers(handle, curve, s, first, n, 0, o)
    for kw, message in [(dict(curve=7), "unknown curve"), (dict(handle=None), "null"), (dict(s=None), "null"), (dict(o=None), "null"),
                        (dict(n=(1 << 32) + 1), "above 2^32"), (dict(first=(1 << 64) - 3, n=8), "above 2^64")]:
        bad(powers(**kw), message)
    assert powers(n=0, s=None, o=None) == 0 and (out == 0xAB).all()
    assert powers(first=(1 << 64) - 8, n=8) == 0 and not (out[:8] == 0xAB).all() and (out[8:] == 0xAB).all()

    for name, call in (("ga_fr_sparse_matvec", valid), ("ga_fr_lagrange_at", lambda: g16_setup.LagrangeAt(ctx, c.name, 16, 5)),
                       ("ga_fr_compact_nonzero", lambda: g16_setup.CompactNonZero(ctx, c.name, xa)), ("ga_fr_powers", lambda: g16_setup.Powers(ctx, c.name, 1, 2, 8))):
        try:
            monkeypatch.setenv("GA_FAULT_THROW", name)
            with pytest.raises(GnarkAmdError, match=r"error -3: out of host memory \(std::bad_alloc\) under " + name):
                call()
            monkeypatch.delenv("GA_FAULT_THROW")
            call()
            valid()
        finally:
            monkeypatch.delenv("GA_FAULT_THROW", raising=False)


# ---- 9. Setup, replayed ---------------------------------------------------------------------------------------------------------------
def setup_matrices(c, cs, mont):
    """pyref.R1CS -> what g16_setup.Setup takes: the wire-major rows of test_phase2_init.wire_major in CSR form"""
    n = 1
    while n < len(cs.L):
        n *= 2
    values, rows_l, rows_r, rows_k = cases.wire_major(cs, n)
    return dict(n=n, nb_wires=cs.nb_wires, nb_public=cs.nb_public, coeffs=words(c, values, mont), montgomery=mont, L=cases.csr(rows_l), R=cases.csr(rows_r),
                LRO=cases.csr(rows_k), commitments=[(cm.private_committed, cm.commitment_index) for cm in cs.commitments])


def general_toxic(c, cs, seed):
    rng = pyref.Xoshiro(seed + c.cid)
    return [rng.field(c.r - 2) + 2 for _ in range(5 + len(cs.commitments) + 1)]   # alpha, beta, gamma, delta, tau, sigmas, the Pedersen G2 dlog


@pytest.mark.parametrize("mont", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("circuit", list(cases.CIRCUITS))
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_setup_replay(emu_ctx, c, circuit, mont):
    """g16_setup.Setup == pyref.groth16_setup(c, cs, toxic) with general alpha, beta, gamma, delta, tau: the scalars against dlog (A, B,
    Z, K, CK) before the point stage, the points A, B, B2, Z (bit-reversed, n - 1 kept), pk.K, vk.K and the commitment bases against the
    oracle's key, infinityA / infinityB and their counts.  "random" has wires missing from L and R; "commit" has all three K classes"""
    ctx = emu_ctx
    cs = cases.CIRCUITS[circuit](c)
    toxic = general_toxic(c, cs, 0x9A11)
    pk, vk, dlog = pyref.groth16_setup(c, cs, toxic)
    key = g16_setup.Setup(ctx, c.name, setup_matrices(c, cs, mont), toxic, keep_scalars=True)
    try:
        n = key.n
        assert n == pk.n
        assert list(key.infinityA) == pk.infinityA and list(key.infinityB) == pk.infinityB
        assert key.len_a == len(pk.A) == cs.nb_wires - sum(pk.infinityA) and key.len_b == len(pk.B) == cs.nb_wires - sum(pk.infinityB)
        if circuit == "random":
            assert any(pk.infinityA) and any(pk.infinityB)
        if circuit == "commit":
            assert key.len_vk > cs.nb_public and key.ck and key.ck[0][2] > 0 and key.len_k > 0

        def scalars(name, count):
            return ints(c, key.scalars[name].to_host((count, 4)), mont) if count else []
        assert scalars("A", key.len_a) == dlog["A"] and scalars("B", key.len_b) == dlog["B"]
        assert pyref.bitrev_permute(scalars("Z", n))[:n - 1] == dlog["Z"]
        assert scalars("K", key.len_k) == dlog["K"]
        assert [scalars("CK%d" % i, len(v)) for i, v in enumerate(dlog["CK"])] == dlog["CK"]

        def pts(buf, group, count):
            return buf.to_host((count, affine_words(c.cid, group))) if count else np.zeros((0, affine_words(c.cid, group)), np.uint64)
        for name, buf, group, want in (("A", key.A, 0, pk.A), ("B", key.B, 0, pk.B), ("B2", key.B2, 1, pk.B2), ("Z", key.Z, 0, pk.Z), ("K", key.K, 0, pk.K),
                                       ("vkK", key.vkK, 0, vk.K)):
            if want:
                cases.check(pts(buf, group, len(want)), pts_to_arr(c, group, want).reshape(len(want), -1), name)
        assert len(key.ck) == len(pk.commitment_keys)
        for (basis, sig, count), (want_basis, want_sig) in zip(key.ck, pk.commitment_keys):
            assert count == len(want_basis) > 0
            cases.check(pts(basis, 0, count), pts_to_arr(c, 0, want_basis).reshape(count, -1), "ck basis")
            cases.check(pts(sig, 0, count), pts_to_arr(c, 0, want_sig).reshape(count, -1), "ck basis exp sigma")
        for name, group, want in (("alpha1", 0, pk.alpha1), ("beta1", 0, pk.beta1), ("delta1", 0, pk.delta1), ("beta2", 1, pk.beta2), ("delta2", 1, pk.delta2),
                                  ("gamma2", 1, vk.gamma2)):
            assert np.array_equal(key.points[name], pts_to_arr(c, group, [want])[0]), name
    finally:
        key.free()


# ---- bindings -------------------------------------------------------------------------------------------------------------------------
def test_setup_symbols_and_go_bindings(emu_lib):
    """the four entry points are exported and bound; ga.go calls them and go/IDENTS.json resolves the calls against the header"""
    go = open(os.path.join(ROOT, "go", "backend", "accelerated", "mi355x", "internal", "ga", "ga.go")).read()
    idents = json.load(open(os.path.join(ROOT, "go", "IDENTS.json")))["resolved"]
    for name, func, nargs in (("ga_fr_lagrange_at", "LagrangeAt", 7), ("ga_fr_sparse_matvec", "SparseMatVec", 14), ("ga_fr_compact_nonzero", "CompactNonZero", 8),
                              ("ga_fr_powers", "Powers", 7)):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(emu_lib, name)
        assert f"func (c *Context) {func}(" in go and f"C.{name}(c.h, C.int(curve)," in go
        assert ["go/backend/accelerated/mi355x/internal/ga/ga.go", f"C.{name}", f"include/gnark_amd.h prototype ({nargs} args)"] in idents

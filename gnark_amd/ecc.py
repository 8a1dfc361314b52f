"""Multi-scalar multiplication -- mirror of gnark-crypto's `G1Jac.MultiExp` / `G2Jac.MultiExp` as the reference
calls them (backend/groth16/bn254/prove.go:194,207,227,237,283), on gnark's own memory images."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .device import Context, DeviceBuffer, _ptr, affine_words, as_u64, curve_id, jac_words

G1, G2 = _lib.G1, _lib.G2


def _arg(x, flag):
    if isinstance(x, DeviceBuffer):
        return C.c_void_p(x.ptr), flag
    if isinstance(x, int):
        return C.c_void_p(x), flag
    return _ptr(x), 0


def MultiExp(ctx: Context, curve, group: int, points, scalars, n: int | None = None, montgomery: bool = True) -> np.ndarray:
    """sum_i scalars[i] * points[i]  ->  one Jacobian point {X,Y,Z} (uint64 limbs, Montgomery).

    points : (n, 2*fp) [G1] or (n, 4*fp) [G2] uint64 array (G1Affine/G2Affine images) or a DeviceBuffer
    scalars: (n, 4) uint64 array (fr.Element images) or a DeviceBuffer
    Errors mirror MultiExp's "len(points) != len(scalars)" check.
    """
    cid = curve_id(curve)
    if not isinstance(points, (DeviceBuffer, int)):
        points = as_u64(points, affine_words(cid, group))
        n_p = points.shape[0]
    else:
        n_p = n
    if not isinstance(scalars, (DeviceBuffer, int)):
        scalars = as_u64(scalars, 4)
        n_s = scalars.shape[0]
    else:
        n_s = n
    if n_p is None or n_s is None:
        raise ValueError("n is required when both operands are device buffers")
    if n_p != n_s:
        raise ValueError("len(points) != len(scalars)")
    bp, f1 = _arg(points, _lib.BASES_ON_DEVICE)
    sp, f2 = _arg(scalars, _lib.SCALARS_ON_DEVICE)
    flags = f1 | f2 | (_lib.SCALARS_MONTGOMERY if montgomery else 0)
    out = np.zeros(jac_words(cid, group), dtype=np.uint64)
    ctx.lib.check(ctx.lib.ga_msm(ctx.handle, cid, group, bp, sp, n_p, flags, _ptr(out)))
    return out


def BatchScalarMultiplication(ctx: Context, curve, group: int, base, scalars, n: int | None = None, montgomery: bool = False,
                              bitreversed: bool = False, out_device: bool = False):
    """[scalars[i]] base for ONE base point -- curve.BatchScalarMultiplicationG1 / G2 as groth16.Setup calls them
    (backend/groth16/bn254/setup.go:233,302) and kzg.NewSRS over the powers of tau.

    base    : one G1Affine / G2Affine image (host array; any point on the curve, (0,0) = infinity)
    scalars : (n, 4) uint64 array or a DeviceBuffer of n elements; canonical integers as gnark's setup passes them, fr.Element
              images with montgomery=True
    bitreversed: result i lands at index bitrev(i, log2 n) (setup.go:247 on the Z points); n must be a power of two
    Returns an (n, affine_words) array, or with out_device=True a DeviceBuffer of n affine points (the caller frees it).
    """
    cid = curve_id(curve)
    wa = affine_words(cid, group)
    base = as_u64(np.asarray(base).reshape(1, -1), wa)
    if not isinstance(scalars, (DeviceBuffer, int)):
        scalars = as_u64(scalars, 4)
        n = scalars.shape[0]
    if n is None:
        raise ValueError("n is required for device-resident scalars")
    sp, f = _arg(scalars, _lib.SCALARS_ON_DEVICE)
    flags = f | (_lib.SCALARS_MONTGOMERY if montgomery else 0) | (_lib.RESULT_BITREVERSED if bitreversed else 0)
    if out_device:
        buf = ctx.malloc(max(n, 1) * wa * 8)
        try:
            ctx.lib.check(ctx.lib.ga_batch_scalar_mul(ctx.handle, cid, group, _ptr(base), sp, n, flags | _lib.RESULT_ON_DEVICE, C.c_void_p(buf.ptr)))
        except Exception:
            buf.free()
            raise
        return buf
    out = np.zeros((n, wa), dtype=np.uint64)
    ctx.lib.check(ctx.lib.ga_batch_scalar_mul(ctx.handle, cid, group, _ptr(base), sp, n, flags, _ptr(out)))
    return out


def batch_scalar_mul_plan(curve, n: int, lib=None):
    """(window_bits, windows) BatchScalarMultiplication uses for n scalars (ga_batch_scalar_mul_plan)"""
    lib = lib or _lib.load()
    c, nw = C.c_int(), C.c_int()
    lib.check(lib.ga_batch_scalar_mul_plan(curve_id(curve), n, C.byref(c), C.byref(nw)))
    return c.value, nw.value


def ToLagrangeG1(ctx: Context, curve, powers, n: int | None = None, out_device: bool = False):
    """kzg.ToLagrangeG1 (gnark-crypto ecc/<curve>/kzg): powers[i] = [tau^i]G1 -> [l_i(tau)]G1 over the size-n domain, natural order.

    powers : (n, affine_words) uint64 array of G1Affine images or a DeviceBuffer of n points (then n is required); never modified
    n must be a power of two (at most 2^28 for BN254, 2^32 for BLS12-381, 2^47 for BLS12-377).  The points are not validated.
    Returns an (n, affine_words) array, or with out_device=True a DeviceBuffer of n affine points (the caller frees it) that
    MultiExp and PrecomputedBases take as they are.
    """
    cid = curve_id(curve)
    wa = affine_words(cid, G1)
    if not isinstance(powers, (DeviceBuffer, int)):
        powers = as_u64(powers, wa)
        n = powers.shape[0]
    if n is None:
        raise ValueError("n is required for device-resident points")
    pp, f = _arg(powers, _lib.BASES_ON_DEVICE)
    if out_device:
        buf = ctx.malloc(max(n, 1) * wa * 8)
        try:
            ctx.lib.check(ctx.lib.ga_kzg_to_lagrange_g1(ctx.handle, cid, pp, n, f | _lib.RESULT_ON_DEVICE, C.c_void_p(buf.ptr)))
        except Exception:
            buf.free()
            raise
        return buf
    out = np.zeros((n, wa), dtype=np.uint64)
    ctx.lib.check(ctx.lib.ga_kzg_to_lagrange_g1(ctx.handle, cid, pp, n, f, _ptr(out)))
    return out


POINT_OK, POINT_OFF_CURVE, POINT_NOT_IN_SUBGROUP = _lib.POINT_OK, _lib.POINT_OFF_CURVE, _lib.POINT_NOT_IN_SUBGROUP
NONE_BAD = 0xFFFFFFFFFFFFFFFF   # `first` when every point is OK


def CheckPoints(ctx: Context, curve, group: int, points, n: int | None = None, curve_only: bool = False, status_device: bool = False,
                status: bool = True):
    """G1Affine / G2Affine.IsOnCurve and IsInSubGroup for a whole vector (ga_check_points) -- what gnark-crypto's default decoder
    does for every point of a ProvingKey.ReadFrom, of the ReadFrom of an mpcsetup phase and of kzg.SRS.ReadFrom.

    points : (n, affine_words) uint64 array of G1Affine / G2Affine images, or a DeviceBuffer of n points (then n is required);
             never written.  Any bytes are accepted: a coordinate that is not below p makes its point POINT_OFF_CURVE.
    curve_only: the curve equation alone (IsOnCurve).
    Returns (status, off_curve, outside, first, redone): status is an (n,) uint8 array of POINT_OK / POINT_OFF_CURVE /
    POINT_NOT_IN_SUBGROUP, a DeviceBuffer of n bytes with status_device=True (the caller frees it), None with status=False;
    off_curve and outside count the two failures, first is the index of the first point that is not OK (NONE_BAD if all are),
    redone counts the points decided by [r]P with the complete formulas (0 on honest input).  Bad points are not an error.
    """
    cid = curve_id(curve)
    wa = affine_words(cid, group)
    if not isinstance(points, (DeviceBuffer, int)):
        points = as_u64(points, wa)
        n = points.shape[0]
    if n is None:
        raise ValueError("n is required for device-resident points")
    pp, flags = _arg(points, _lib.BASES_ON_DEVICE)
    if curve_only:
        flags |= _lib.CHECK_CURVE_ONLY
    out4 = (C.c_uint64 * 4)()
    res, sp = None, C.c_void_p(None)
    if status and status_device:
        res = ctx.malloc(max(n, 1))
        sp, flags = C.c_void_p(res.ptr), flags | _lib.RESULT_ON_DEVICE
    elif status:
        res = np.zeros(n, dtype=np.uint8)
        sp = _ptr(res)
    try:
        ctx.lib.check(ctx.lib.ga_check_points(ctx.handle, cid, group, pp, n, flags, sp, out4))
    except Exception:
        if isinstance(res, DeviceBuffer):
            res.free()
        raise
    return res, int(out4[0]), int(out4[1]), int(out4[2]), int(out4[3])


def PairingCheck(ctx: Context, curve, P, Q, group_start=None, *, n: int | None = None, want_gt: bool = False, on_device: bool = False):
    """prod_{i in group g} e(P_i, Q_i) == 1 for every group of a vector of pairs (ga_pairing_check) -- curve.PairingCheck as the
    Groth16 verifier, pedersen.BatchVerifyMultiVk, kzg.Verify and mpcsetup's SameRatio call it, for many equations in one call.

    P, Q        : (n, affine_words) uint64 arrays of G1Affine / G2Affine images, or both DeviceBuffers of n points (n then comes
                  from group_start, or from `n`); never written.  (0,0) on either side of a pair contributes 1.  The points are
                  not validated (CheckPoints does that).
    group_start : n_groups + 1 offsets (0, ..., n), non-decreasing; None = one group of all pairs.
    Returns (ok, bad, first), with want_gt=True (ok, gt, bad, first): ok is an (n_groups,) uint8 array of 0 / 1, gt an
    (n_groups, 12 * fp_words) uint64 array of E12 memory images (the library's own normalisation of e: see include/gnark_amd.h) --
    with on_device=True both are DeviceBuffers (the caller frees them); bad counts the groups whose product is not 1 and first is
    the index of the first of them (NONE_BAD if there is none).
    """
    cid = curve_id(curve)
    w1, w2 = affine_words(cid, G1), affine_words(cid, G2)
    dev = isinstance(P, (DeviceBuffer, int))
    if dev != isinstance(Q, (DeviceBuffer, int)):
        raise ValueError("P and Q are both host arrays or both device buffers")
    gs = None
    if group_start is not None:
        gs = np.ascontiguousarray(group_start, dtype=np.uint64).reshape(-1)
        if gs.size < 1:
            raise ValueError("group_start holds n_groups + 1 offsets")
    if not dev:
        P, Q = as_u64(P, w1), as_u64(Q, w2)
        if P.shape[0] != Q.shape[0]:
            raise ValueError("len(P) != len(Q)")
        n = P.shape[0]
    elif n is None:
        if gs is None:
            raise ValueError("n or group_start is required for device-resident points")
        n = int(gs[-1])
    n_groups = 1 if gs is None else gs.size - 1
    pp, flags = _arg(P, _lib.BASES_ON_DEVICE)
    qp, _ = _arg(Q, _lib.BASES_ON_DEVICE)
    wg = 6 * w1   # 12 base-field elements
    out2 = (C.c_uint64 * 2)(0, NONE_BAD)
    ok = gt = None
    try:
        if on_device:
            flags |= _lib.RESULT_ON_DEVICE
            ok = ctx.malloc(max(n_groups, 1))
            gt = ctx.malloc(max(n_groups, 1) * wg * 8) if want_gt else None
            okp, gtp = C.c_void_p(ok.ptr), C.c_void_p(gt.ptr if gt else None)
        else:
            ok = np.zeros(n_groups, dtype=np.uint8)
            gt = np.zeros((n_groups, wg), dtype=np.uint64) if want_gt else None
            okp, gtp = _ptr(ok), (_ptr(gt) if want_gt else C.c_void_p(None))
        ctx.lib.check(ctx.lib.ga_pairing_check(ctx.handle, cid, pp, qp, n, _ptr(gs) if gs is not None else C.c_void_p(None), n_groups, flags, okp, gtp, out2))
    except Exception:
        for b in (ok, gt):
            if isinstance(b, DeviceBuffer):
                b.free()
        raise
    return (ok, gt, int(out2[0]), int(out2[1])) if want_gt else (ok, int(out2[0]), int(out2[1]))


def ScalePoints(ctx: Context, curve, group: int, points, scalars=None, *, scalar=None, powers=None, first: int = 0, n: int | None = None,
                montgomery: bool = False, out_device: bool = False, in_place: bool = False):
    """out[i] = [s_i] points[i] -- the ScalarMultiplication loops of the Groth16 MPC ceremony (backend/groth16/<curve>/mpcsetup:
    SrsCommons.update, Phase2.update) as one call (ga_scale_points).  Exactly one of
      scalars      : (n, 4) uint64 array or a DeviceBuffer of n elements   s_i = scalars[i]
      scalar       : one element (int, or 4 uint64 words)                  s_i = scalar
      powers=(c, t): two elements                                          s_i = c * t^(first + i)
    Elements are canonical integers, fr.Element images with montgomery=True (ints are always canonical: pass words for images).

    points : (n, affine_words) uint64 array of G1Affine / G2Affine images, or a DeviceBuffer of n points (then n is required).
    in_place: the result overwrites `points` (a DeviceBuffer: the same buffer is returned; an array: the array is written and
    returned); otherwise `points` is never written.  The points are not validated.
    Returns (array | DeviceBuffer, redone): redone counts the points that took the complete formulas (0 for an honest SRS).
    """
    cid = curve_id(curve)
    wa = affine_words(cid, group)
    if sum(x is not None for x in (scalars, scalar, powers)) != 1:
        raise ValueError("exactly one of scalars, scalar and powers=(c, t) must be given")
    on_dev = isinstance(points, (DeviceBuffer, int))
    if not on_dev:
        points = as_u64(points, wa)
        n = points.shape[0]
    if n is None:
        raise ValueError("n is required for device-resident points")

    def words(k):
        if isinstance(k, (int, np.integer)):
            return [(int(k) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
        return list(np.asarray(k, dtype=np.uint64).reshape(4))

    sflag = 0
    if scalars is not None:
        mode = _lib.SCALE_EACH
        if not isinstance(scalars, (DeviceBuffer, int)):
            scalars = as_u64(scalars, 4)
            if scalars.shape[0] != n:
                raise ValueError("len(points) != len(scalars)")
        sp, sflag = _arg(scalars, _lib.SCALARS_ON_DEVICE)
    else:
        mode = _lib.SCALE_ONE if scalar is not None else _lib.SCALE_POWERS
        keep = np.array([words(k) for k in ([scalar] if scalar is not None else list(powers))], dtype=np.uint64)
        if keep.shape != ((1, 4) if scalar is not None else (2, 4)):
            raise ValueError("powers takes two elements (c, t)")
        sp = _ptr(keep)
    pp, pflag = _arg(points, _lib.BASES_ON_DEVICE)
    flags = pflag | sflag | (_lib.SCALARS_MONTGOMERY if montgomery else 0)
    redone = C.c_uint64(0)

    def run(out_ptr, oflag):
        ctx.lib.check(ctx.lib.ga_scale_points(ctx.handle, cid, group, pp, n, mode, sp, int(first), flags | oflag, out_ptr, C.byref(redone)))

    if in_place:
        if out_device != on_dev and out_device:
            raise ValueError("in_place with out_device needs device-resident points")
        run(pp, _lib.RESULT_ON_DEVICE if on_dev else 0)
        return points, redone.value
    if out_device:
        buf = ctx.malloc(max(n, 1) * wa * 8)
        try:
            run(C.c_void_p(buf.ptr), _lib.RESULT_ON_DEVICE)
        except Exception:
            buf.free()
            raise
        return buf, redone.value
    out = np.zeros((n, wa), dtype=np.uint64)
    run(_ptr(out), 0)
    return out, redone.value


def LagrangeCoeffs(ctx: Context, curve, group: int, powers, n: int | None = None, out_device: bool = False):
    """lagrangeCoeffsG1 / lagrangeCoeffsG2 of the Groth16 MPC ceremony (backend/groth16/<curve>/mpcsetup/lagrange.go): the inverse
    FFT over n points of G1 or G2, natural order in and out (ga_lagrange_coeffs).  group = G1 gives the bytes of ToLagrangeG1.

    powers : (n, affine_words) uint64 array of G1Affine / G2Affine images or a DeviceBuffer of n points (then n is required); never
    modified.  n must be a power of two (at most 2^28 for BN254, 2^32 for BLS12-381, 2^47 for BLS12-377).  The points are not validated.
    Returns an (n, affine_words) array, or with out_device=True a DeviceBuffer of n affine points (the caller frees it).
    """
    cid = curve_id(curve)
    wa = affine_words(cid, group)
    if not isinstance(powers, (DeviceBuffer, int)):
        powers = as_u64(powers, wa)
        n = powers.shape[0]
    if n is None:
        raise ValueError("n is required for device-resident points")
    pp, f = _arg(powers, _lib.BASES_ON_DEVICE)
    if out_device:
        buf = ctx.malloc(max(n, 1) * wa * 8)
        try:
            ctx.lib.check(ctx.lib.ga_lagrange_coeffs(ctx.handle, cid, group, pp, n, f | _lib.RESULT_ON_DEVICE, C.c_void_p(buf.ptr)))
        except Exception:
            buf.free()
            raise
        return buf
    out = np.zeros((n, wa), dtype=np.uint64)
    ctx.lib.check(ctx.lib.ga_lagrange_coeffs(ctx.handle, cid, group, pp, n, f, _ptr(out)))
    return out


def SparsePointSums(ctx: Context, curve, group: int, points, row_start, terms, coeffs, *, montgomery: bool = False, bitreversed: bool = False,
                    n_points: int | None = None, out_device: bool = False):
    """out[r] = sum_k [coeffs[cid_k]] points[col_k] over the terms k of row r -- a sparse Fr matrix in CSR form applied to a vector of
    points: the constraint loop of the Groth16 MPC ceremony's Phase2.Initialize (ga_sparse_point_sums).

    points    : (n_points, affine_words) uint64 array of G1Affine / G2Affine images, or a DeviceBuffer (then n_points is required)
    row_start : n_rows + 1 offsets into terms, row_start[0] = 0, row_start[-1] = len(terms)
    terms     : (nnz, 2) uint32 {cid, col} pairs, row after row (constraint.Term's memory image with the column in VID)
    coeffs    : (n_coeffs, 4) uint64 elements, canonical integers (any 256-bit value: reduced), fr.Element images with montgomery=True
    bitreversed: row r lands at index bitrev(r, log2 n_rows); n_rows must be a power of two
    Returns (array | DeviceBuffer of n_rows affine points, redone): redone counts the products and row segments that took the complete
    formulas (repeated or cancelling operands); the result is exact either way.  An empty row and a cancelled sum are (0,0).
    """
    cid = curve_id(curve)
    wa = affine_words(cid, group)
    if not isinstance(points, (DeviceBuffer, int)):
        points = as_u64(points, wa)
        n_points = points.shape[0]
    if n_points is None:
        raise ValueError("n_points is required for device-resident points")
    row_start = np.ascontiguousarray(row_start, dtype=np.uint64).reshape(-1)
    if row_start.size == 0:
        raise ValueError("row_start holds n_rows + 1 offsets")
    n_rows = row_start.size - 1
    terms = np.ascontiguousarray(terms, dtype=np.uint32).reshape(-1, 2)
    if terms.shape[0] != int(row_start[-1]):
        raise ValueError("len(terms) != row_start[-1]")
    coeffs = as_u64(coeffs, 4)
    pp, pflag = _arg(points, _lib.BASES_ON_DEVICE)
    flags = pflag | (_lib.SCALARS_MONTGOMERY if montgomery else 0) | (_lib.RESULT_BITREVERSED if bitreversed else 0)
    redone = C.c_uint64(0)

    def run(out_ptr, oflag):
        ctx.lib.check(ctx.lib.ga_sparse_point_sums(ctx.handle, cid, group, pp, n_points, _ptr(row_start), n_rows, _ptr(terms), _ptr(coeffs),
                                                   coeffs.shape[0], flags | oflag, out_ptr, C.byref(redone)))

    if out_device:
        buf = ctx.malloc(max(n_rows, 1) * wa * 8)
        try:
            run(C.c_void_p(buf.ptr), _lib.RESULT_ON_DEVICE)
        except Exception:
            buf.free()
            raise
        return buf, redone.value
    out = np.zeros((n_rows, wa), dtype=np.uint64)
    run(_ptr(out), 0)
    return out, redone.value


class PrecomputedBases:
    """Bases pinned on the device together with [2^(c*w)]P for every Pippenger window w (ga_msm_table_*): the GPU analogue of
    keeping `pk.G1.A` etc. resident ("PinToGPU", provingkey.go:37-42) with ICICLE's PrecomputeFactor."""

    def __init__(self, ctx: Context, curve, group: int, points, n: int | None = None, batched: bool = False):
        """batched: the table will mostly serve MultiExpBatch (GA_TABLE_BATCHED: a narrower window is planned)"""
        cid = curve_id(curve)
        if not isinstance(points, (DeviceBuffer, int)):
            points = as_u64(points, affine_words(cid, group))
            n = points.shape[0]
        if n is None:
            raise ValueError("n is required for device-resident points")
        bp, f1 = _arg(points, _lib.BASES_ON_DEVICE)
        h = C.c_void_p()
        ctx.lib.check(ctx.lib.ga_msm_table_create(ctx.handle, cid, group, bp, n, f1 | (_lib.TABLE_BATCHED if batched else 0), C.byref(h)))
        self.ctx, self.curve, self.group, self.n, self.handle = ctx, cid, group, n, h

    def info(self):
        c, nw, nb = C.c_int(), C.c_int(), C.c_uint64()
        self.ctx.lib.check(self.ctx.lib.ga_msm_table_info(self.handle, C.byref(c), C.byref(nw), C.byref(nb)))
        return {"window_bits": c.value, "windows": nw.value, "table_bytes": nb.value}

    def MultiExpWindows(self, scalars, win_lo: int, win_hi: int, montgomery: bool = True) -> np.ndarray:
        """windows [win_lo, win_hi) only (ga_msm_table_run_windows): partial results of disjoint ranges add up to MultiExp's"""
        if not isinstance(scalars, (DeviceBuffer, int)):
            scalars = as_u64(scalars, 4)
            if scalars.shape[0] != self.n:
                raise ValueError("len(points) != len(scalars)")
        sp, f2 = _arg(scalars, _lib.SCALARS_ON_DEVICE)
        out = np.zeros(jac_words(self.curve, self.group), dtype=np.uint64)
        flags = f2 | (_lib.SCALARS_MONTGOMERY if montgomery else 0)
        self.ctx.lib.check(self.ctx.lib.ga_msm_table_run_windows(self.handle, sp, flags, int(win_lo), int(win_hi), _ptr(out)))
        return out

    def MultiExp(self, scalars, montgomery: bool = True) -> np.ndarray:
        if not isinstance(scalars, (DeviceBuffer, int)):
            scalars = as_u64(scalars, 4)
            if scalars.shape[0] != self.n:
                raise ValueError("len(points) != len(scalars)")
        sp, f2 = _arg(scalars, _lib.SCALARS_ON_DEVICE)
        out = np.zeros(jac_words(self.curve, self.group), dtype=np.uint64)
        self.ctx.lib.check(self.ctx.lib.ga_msm_table_run(self.handle, sp, f2 | (_lib.SCALARS_MONTGOMERY if montgomery else 0), _ptr(out)))
        return out

    def MultiExpBatch(self, scalar_vectors, montgomery: bool = True) -> np.ndarray:
        """k scalar vectors over these bases in one pass (ga_msm_table_run_batch): (k, jac_words) -- row j equals MultiExp(vector j).
        All vectors host arrays or all DeviceBuffers."""
        k = len(scalar_vectors)
        on_dev = all(isinstance(v, (DeviceBuffer, int)) for v in scalar_vectors)
        if not on_dev:
            if any(isinstance(v, (DeviceBuffer, int)) for v in scalar_vectors):
                raise ValueError("a batch mixes host and device scalar vectors")
            scalar_vectors = [as_u64(v, 4) for v in scalar_vectors]
            if any(v.shape[0] != self.n for v in scalar_vectors):
                raise ValueError("len(points) != len(scalars)")
        ptrs, flags = [], (_lib.SCALARS_MONTGOMERY if montgomery else 0)
        for v in scalar_vectors:
            p, f = _arg(v, _lib.SCALARS_ON_DEVICE)
            ptrs.append(p)
            flags |= f
        arr = (C.c_void_p * k)(*[C.cast(p, C.c_void_p).value for p in ptrs])
        out = np.zeros((k, jac_words(self.curve, self.group)), dtype=np.uint64)
        self.ctx.lib.check(self.ctx.lib.ga_msm_table_run_batch(self.handle, arr, k, flags, _ptr(out)))
        return out

    def KzgOpen(self, poly, point):
        """kzg.Open(p, point, pk) over this (monomial G1) SRS: returns (ClaimedValue fr image, H as G1Jac)."""
        n = None
        if not isinstance(poly, (DeviceBuffer, int)):
            poly = as_u64(poly, 4)
            n = poly.shape[0]
        else:
            raise ValueError("pass the coefficient array (host); device polynomials go through ga_kzg_open directly")
        pp, f = _arg(poly, _lib.SCALARS_ON_DEVICE)
        z = as_u64(np.asarray(point).reshape(1, 4), 4)
        val = np.zeros(4, dtype=np.uint64)
        out = np.zeros(jac_words(self.curve, self.group), dtype=np.uint64)
        self.ctx.lib.check(self.ctx.lib.ga_kzg_open(self.handle, pp, n, f, _ptr(z), _ptr(val), _ptr(out)))
        return val, out

    def KzgOpenBatch(self, polys, points):
        """kzg.Open for many polynomials of one length over this SRS in one call (ga_kzg_open_batch): polys is a sequence of
        coefficient arrays (host) or a (count, n, 4) array, points (count, 4).  Returns (ClaimedValues (count, 4), H (count, jac_words));
        item j is KzgOpen(polys[j], points[j])."""
        ps = [as_u64(np.asarray(p).reshape(-1, 4), 4) for p in polys]
        count = len(ps)
        z = as_u64(np.asarray(points).reshape(-1, 4), 4)
        if z.shape[0] != count or any(p.shape != ps[0].shape for p in ps):
            raise ValueError("one point per polynomial, polynomials of equal length")
        vals = np.zeros((count, 4), dtype=np.uint64)
        out = np.zeros((count, jac_words(self.curve, self.group)), dtype=np.uint64)
        if count:
            arr = (C.c_void_p * count)(*[p.ctypes.data for p in ps])
            self.ctx.lib.check(self.ctx.lib.ga_kzg_open_batch(self.handle, arr, ps[0].shape[0], count, 0, _ptr(z), _ptr(vals), _ptr(out)))
        return vals, out

    def free(self):
        if self.handle:
            self.ctx.lib.ga_msm_table_destroy(self.handle)
            self.handle = None


def MultiExpWindows(ctx: Context, curve, group: int, points, scalars, n: int, win_lo: int, win_hi: int, montgomery=True):
    """Window-sharded MSM (multi-GPU partitioning A): Jacobian window sums for windows [win_lo, win_hi)."""
    cid = curve_id(curve)
    c, nw = plan(curve, group, n, lib=ctx.lib)
    hi = nw if win_hi < 0 else win_hi
    if not isinstance(points, (DeviceBuffer, int)):
        points = as_u64(points, affine_words(cid, group))
    if not isinstance(scalars, (DeviceBuffer, int)):
        scalars = as_u64(scalars, 4)
    bp, f1 = _arg(points, _lib.BASES_ON_DEVICE)
    sp, f2 = _arg(scalars, _lib.SCALARS_ON_DEVICE)
    flags = f1 | f2 | (_lib.SCALARS_MONTGOMERY if montgomery else 0)
    out = np.zeros((hi - win_lo, jac_words(cid, group)), dtype=np.uint64)
    cc, nn = C.c_int(), C.c_int()
    ctx.lib.check(ctx.lib.ga_msm_windows(ctx.handle, cid, group, bp, sp, n, flags, win_lo, win_hi, _ptr(out), C.byref(cc), C.byref(nn)))
    return out, cc.value, nn.value


def plan(curve, group: int, n: int, lib=None):
    lib = lib or _lib.load()
    c, nw = C.c_int(), C.c_int()
    lib.check(lib.ga_msm_plan(curve_id(curve), group, n, C.byref(c), C.byref(nw)))
    return c.value, nw.value


def combine_windows(curve, group: int, windows: np.ndarray, window_bits: int, lib=None) -> np.ndarray:
    lib = lib or _lib.load()
    cid = curve_id(curve)
    windows = as_u64(windows, jac_words(cid, group))
    out = np.zeros(jac_words(cid, group), dtype=np.uint64)
    lib.check(lib.ga_msm_combine_windows(cid, group, _ptr(windows), windows.shape[0], window_bits, _ptr(out)))
    return out


def jac_add(curve, group, a, b, lib=None):
    lib = lib or _lib.load()
    cid = curve_id(curve)
    a, b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
    out = np.zeros(jac_words(cid, group), dtype=np.uint64)
    lib.check(lib.ga_jac_add(cid, group, _ptr(a), _ptr(b), _ptr(out)))
    return out


def jac_to_affine(curve, group, a, lib=None):
    lib = lib or _lib.load()
    cid = curve_id(curve)
    a = np.ascontiguousarray(a, dtype=np.uint64)
    out = np.zeros(affine_words(cid, group), dtype=np.uint64)
    lib.check(lib.ga_jac_to_affine(cid, group, _ptr(a), _ptr(out)))
    return out


def jac_scalar_mul(curve, group, a, k_canonical: int, lib=None):
    lib = lib or _lib.load()
    cid = curve_id(curve)
    a = np.ascontiguousarray(a, dtype=np.uint64)
    k = np.array([(k_canonical >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
    out = np.zeros(jac_words(cid, group), dtype=np.uint64)
    lib.check(lib.ga_jac_scalar_mul(cid, group, _ptr(a), _ptr(k), _ptr(out)))
    return out


def generator_mul(curve, group, k_canonical: int, lib=None):
    lib = lib or _lib.load()
    cid = curve_id(curve)
    k = np.array([(k_canonical >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
    out = np.zeros(jac_words(cid, group), dtype=np.uint64)
    lib.check(lib.ga_generator_mul(cid, group, _ptr(k), _ptr(out)))
    return out

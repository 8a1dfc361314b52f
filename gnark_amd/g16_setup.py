"""The scalar side of groth16.Setup on the device (backend/groth16/bn254/setup.go:75-331): the four Fr vector calls ga_fr_lagrange_at,
ga_fr_sparse_matvec, ga_fr_compact_nonzero and ga_fr_powers as thin wrappers in the style of ecc.py, and Setup, which chains them with
BatchScalarMultiplication so that no scalar and no point of the key crosses PCIe."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, ecc
from .device import Context, DeviceBuffer, _ptr, as_u64, curve_id
from .ecc import G1, G2, _arg

FR_MODULUS = {
    _lib.BN254: 21888242871839275222246405745257275088548364400416034343698204186575808495617,
    _lib.BLS12_381: 52435875175126190479447740508185965837690552500527637822603658699938581184513,
}


def _words(k: int):
    return [(int(k) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def _elements(cid: int, ks, montgomery: bool) -> np.ndarray:
    """ints (canonical) -> (len, 4) uint64 elements in the form the flag names; arrays of words pass through"""
    if isinstance(ks, np.ndarray):
        return as_u64(ks.reshape(-1, 4), 4)
    r = FR_MODULUS[cid]
    return np.array([_words((int(k) << 256) % r if montgomery else k) for k in ks], dtype=np.uint64).reshape(-1, 4)


def _out(ctx, n, out_device, run):
    """run(pointer, flag) into a fresh DeviceBuffer or array of n elements"""
    if out_device:
        buf = ctx.malloc(max(n, 1) * 32)
        try:
            run(C.c_void_p(buf.ptr), _lib.RESULT_ON_DEVICE)
        except Exception:
            buf.free()
            raise
        return buf
    out = np.zeros((n, 4), dtype=np.uint64)
    run(_ptr(out), 0)
    return out


def LagrangeAt(ctx: Context, curve, n: int, tau, m: int | None = None, *, montgomery: bool = False, out_device: bool = False):
    """out[i] = L_i(tau), i < m <= n: the Lagrange basis of the size-n domain at one point (ga_fr_lagrange_at; setup.go:356-421).
    tau: an int (canonical) or 4 uint64 words in the form `montgomery` names.  Returns an (m, 4) array or a DeviceBuffer."""
    cid = curve_id(curve)
    m = n if m is None else m
    t = _elements(cid, tau if isinstance(tau, np.ndarray) else [tau], montgomery)
    mflag = _lib.SCALARS_MONTGOMERY if montgomery else 0
    return _out(ctx, m, out_device, lambda p, f: ctx.lib.check(ctx.lib.ga_fr_lagrange_at(ctx.handle, cid, n, _ptr(t), m, mflag | f, p)))


def SparseMatVec(ctx: Context, curve, x, row_start, terms, coeffs, *, row_class=None, row_scales=None, montgomery: bool = False,
                 n_cols: int | None = None, out_device: bool = False):
    """out[r] = s_r * sum_k coeffs[cid_k] * x[col_k] over the terms k of row r -- a sparse Fr matrix in CSR form applied to an Fr
    vector (ga_fr_sparse_matvec; the term loops of setupABC and the K loop of setup.go).

    x         : (n_cols, 4) uint64 array or a DeviceBuffer (then n_cols is required)
    row_start, terms, coeffs : as ecc.SparsePointSums takes them
    row_class : n_rows bytes, row_scales : (n_classes, 4) elements; s_r = row_scales[row_class[r]]; both None: s_r = 1
    Every element is canonical (any 256-bit value: reduced), or an fr.Element image with montgomery=True; so is the output.
    """
    cid = curve_id(curve)
    if not isinstance(x, (DeviceBuffer, int)):
        x = as_u64(x, 4)
        n_cols = x.shape[0]
    if n_cols is None:
        raise ValueError("n_cols is required for a device-resident vector")
    row_start = np.ascontiguousarray(row_start, dtype=np.uint64).reshape(-1)
    if row_start.size == 0:
        raise ValueError("row_start holds n_rows + 1 offsets")
    n_rows = row_start.size - 1
    terms = np.ascontiguousarray(terms, dtype=np.uint32).reshape(-1, 2)
    if terms.shape[0] != int(row_start[-1]):
        raise ValueError("len(terms) != row_start[-1]")
    coeffs = as_u64(coeffs, 4)
    if (row_class is None) != (row_scales is None):
        raise ValueError("row_class and row_scales come together")
    cp = sp = None
    n_classes = 0
    if row_class is not None:
        row_class = np.ascontiguousarray(row_class, dtype=np.uint8).reshape(-1)
        if row_class.size != n_rows:
            raise ValueError("len(row_class) != n_rows")
        row_scales = as_u64(row_scales, 4)
        cp, sp, n_classes = _ptr(row_class), _ptr(row_scales), row_scales.shape[0]
    xp, xflag = _arg(x, _lib.VECTOR_ON_DEVICE)
    flags = xflag | (_lib.SCALARS_MONTGOMERY if montgomery else 0)
    return _out(ctx, n_rows, out_device, lambda p, f: ctx.lib.check(ctx.lib.ga_fr_sparse_matvec(
        ctx.handle, cid, xp, n_cols, _ptr(row_start), n_rows, _ptr(terms), _ptr(coeffs), coeffs.shape[0], cp, sp, n_classes, flags | f, p)))


def CompactNonZero(ctx: Context, curve, v, n: int | None = None, *, in_place: bool = False, out_device: bool = False, mask: bool = True):
    """the zero filter of setup.go:195-219 (ga_fr_compact_nonzero): the non-zero elements of v in order.

    v : (n, 4) uint64 array or a DeviceBuffer of n elements (then n is required).  in_place: the result overwrites the head of v
    (the same buffer or array is returned).  Returns (out, mask, count): out is an (n, 4) array / a DeviceBuffer of n elements whose
    first `count` elements are the result; mask[i] is True where v[i] == 0 (None with mask=False)."""
    cid = curve_id(curve)
    on_dev = isinstance(v, (DeviceBuffer, int))
    if not on_dev:
        v = as_u64(v, 4)
        n = v.shape[0]
    if n is None:
        raise ValueError("n is required for a device-resident vector")
    vp, vflag = _arg(v, _lib.VECTOR_ON_DEVICE)
    m = np.zeros(n, dtype=np.uint8) if mask else None
    count = C.c_uint64(0)

    def run(p, f):
        ctx.lib.check(ctx.lib.ga_fr_compact_nonzero(ctx.handle, cid, vp, n, vflag | f, p, None if m is None else _ptr(m), C.byref(count)))

    if in_place:
        run(vp, _lib.RESULT_ON_DEVICE if on_dev else 0)
        out = v
    else:
        out = _out(ctx, n, out_device, run)
    return out, (None if m is None else m.astype(bool)), count.value


def Powers(ctx: Context, curve, c, t, n: int, first: int = 0, *, montgomery: bool = False, out_device: bool = False):
    """out[i] = c * t^(first + i), i < n (ga_fr_powers): the Z scalars of setup.go:181-192, the powers of tau of kzg.NewSRS.
    c, t: ints (canonical) or 4 uint64 words each in the form `montgomery` names."""
    cid = curve_id(curve)
    ct = np.concatenate([_elements(cid, k if isinstance(k, np.ndarray) else [k], montgomery) for k in (c, t)])
    mflag = _lib.SCALARS_MONTGOMERY if montgomery else 0
    return _out(ctx, n, out_device, lambda p, f: ctx.lib.check(ctx.lib.ga_fr_powers(ctx.handle, cid, _ptr(ct), int(first), n, mflag | f, p)))


class SetupKey:
    """What Setup leaves on the device.  Vectors are DeviceBuffers of affine points, ready for ga_g16_builder_append /
    PrecomputedBases(..., n=len): A, B (G1), B2 (G2), each `len_a` / `len_b` points (zeros filtered); Z: n - 1 points, bit-reversed; K:
    pk.G1.K; vkK: vk.G1.K; ck: [(Basis, BasisExpSigma, len)] per commitment.  infinityA / infinityB: bool arrays over the wires.
    points: the single points alpha1, beta1, delta1 (G1), beta2, delta2, gamma2 (G2) as host arrays.  scalars: the Fr vectors behind the
    point vectors (A, B compacted, Z natural order, K, vkK, CK<i>), kept when Setup is called with keep_scalars=True."""

    def __init__(self):
        self.n = self.nb_wires = self.len_a = self.len_b = self.len_k = self.len_vk = 0
        self.A = self.B = self.B2 = self.Z = self.K = self.vkK = None
        self.ck, self.points, self.scalars = [], {}, {}
        self.infinityA = self.infinityB = None

    def buffers(self):
        out = [self.A, self.B, self.B2, self.Z, self.K, self.vkK] + [b for basis, sig, _ in self.ck for b in (basis, sig)] + list(self.scalars.values())
        return [b for b in out if isinstance(b, DeviceBuffer)]

    def free(self):
        for b in self.buffers():
            b.free()


def Setup(ctx: Context, curve, matrices: dict, toxic, *, keep_scalars: bool = False) -> SetupKey:
    """groth16.Setup from (toxic waste, R1CS matrices) to device-resident key vectors.

    matrices: dict with
      n            the domain size (a power of two >= the number of constraints), nb_wires, nb_public
      coeffs       (n_coeffs, 4) r1cs.Coefficients, `montgomery` (bool, default True) says in which form
      L, R, LRO    (row_start, terms) each, wire-major: the rows of wire w hold its terms {cid, constraint}; LRO holds the terms of L,
                   R and O with column offsets 0, n and 2n (the counting sort of INTEGRATION.md)
      commitments  [(private_committed wire ids, commitment wire id)] (constraint.Groth16Commitments); default none
    toxic: ints alpha, beta, gamma, delta, tau, then one sigma per commitment (sampling them is the caller's business).
    """
    cid = curve_id(curve)
    r = FR_MODULUS[cid]
    lib, h = ctx.lib, ctx.handle
    n, nw, nb_public = int(matrices["n"]), int(matrices["nb_wires"]), int(matrices["nb_public"])
    mont = bool(matrices.get("montgomery", True))
    mflag = _lib.SCALARS_MONTGOMERY if mont else 0
    coeffs = as_u64(matrices["coeffs"], 4)
    commitments = list(matrices.get("commitments", []))
    alpha, beta, gamma, delta, tau = (int(k) % r for k in toxic[:5])
    sigmas = [int(k) % r for k in toxic[5:5 + len(commitments)]]
    if len(sigmas) != len(commitments):
        raise ValueError("one sigma per commitment after (alpha, beta, gamma, delta, tau)")
    dinv, ginv = pow(delta, -1, r), pow(gamma, -1, r)
    key = SetupKey()
    key.n, key.nb_wires = n, nw
    tmp = {}
    one = _elements(cid, [1], mont)
    # the group generators as affine images: [1]G (host arithmetic of the library)
    gens = {g: ecc.jac_to_affine(cid, g, ecc.generator_mul(cid, g, 1, lib=lib), lib=lib).reshape(1, -1) for g in (G1, G2)}

    def gather(src, idx):
        """src[idx] as a selection matrix: rows of one term with coefficient 1"""
        idx = np.asarray(idx, dtype=np.uint32)
        terms = np.stack([np.zeros_like(idx), idx], axis=1) if idx.size else np.zeros((0, 2), np.uint32)
        return SparseMatVec(ctx, cid, src, np.arange(idx.size + 1, dtype=np.uint64), terms, one, montgomery=mont, n_cols=nw, out_device=True)

    def points(group, scalars, count, **kw):
        return ecc.BatchScalarMultiplication(ctx, cid, group, gens[group], scalars, n=count, montgomery=mont, out_device=True, **kw)

    try:
        # [beta lag | alpha lag | lag]: the Lagrange values land in the third block, the other two are scaled copies
        cat = tmp["cat"] = ctx.malloc(3 * n * 32)
        lag = cat.offset(2 * n * 32)
        t = _elements(cid, [tau], mont)
        lib.check(lib.ga_fr_lagrange_at(h, cid, n, _ptr(t), n, mflag | _lib.RESULT_ON_DEVICE, C.c_void_p(lag)))
        vecs = (C.c_void_p * 1)(lag)
        for j, k in enumerate((beta, alpha)):
            s = _elements(cid, [k], True)   # (the scalar of a linear combination is always an fr.Element image)
            lib.check(lib.ga_fr_linear_combination(h, cid, n, 1, vecs, _ptr(s), C.c_void_p(cat.offset(j * n * 32)), 1))
        a_full = tmp["a"] = SparseMatVec(ctx, cid, lag, *matrices["L"], coeffs, montgomery=mont, n_cols=n, out_device=True)
        b_full = tmp["b"] = SparseMatVec(ctx, cid, lag, *matrices["R"], coeffs, montgomery=mont, n_cols=n, out_device=True)
        # K: / gamma for public, commitment and private-committed wires, / delta for the rest (setup.go:154-178)
        com_wires = {int(w) for _, w in commitments}
        owner = {int(w): ci for ci, (private, _) in enumerate(commitments) for w in private}
        row_class = np.array([1 if (w < nb_public or w in com_wires or w in owner) else 0 for w in range(nw)], dtype=np.uint8)
        k_full = tmp["k"] = SparseMatVec(ctx, cid, cat, *matrices["LRO"], coeffs, row_class=row_class, row_scales=_elements(cid, [dinv, ginv], mont),
                                         montgomery=mont, n_cols=3 * n, out_device=True)
        vk_idx = [w for w in range(nw) if w < nb_public or w in com_wires]
        pk_idx = [w for w in range(nw) if row_class[w] == 0]
        ck_idx = [[int(w) for w in private] for private, _ in commitments]
        groups = [gather(k_full, idx) for idx in [pk_idx, vk_idx] + ck_idx]
        for i, g in enumerate(groups):
            tmp["g%d" % i] = g
        _, mask_a, key.len_a = CompactNonZero(ctx, cid, a_full, nw, in_place=True)
        _, mask_b, key.len_b = CompactNonZero(ctx, cid, b_full, nw, in_place=True)
        key.infinityA, key.infinityB = mask_a, mask_b
        tn1 = (pow(tau, n, r) - 1) % r
        z = tmp["z"] = Powers(ctx, cid, tn1 * dinv % r, tau, n, montgomery=mont, out_device=True)
        # the point stage: scalars and results stay on the device
        key.A = points(G1, a_full, key.len_a)
        key.B = points(G1, b_full, key.len_b)
        key.B2 = points(G2, b_full, key.len_b)
        key.Z = points(G1, z, n, bitreversed=True)   # n - 1 kept (setup.go:247-249)
        key.len_k, key.len_vk = len(pk_idx), len(vk_idx)
        key.K = points(G1, groups[0], key.len_k)
        key.vkK = points(G1, groups[1], key.len_vk)
        for ci, idx in enumerate(ck_idx):
            basis = points(G1, groups[2 + ci], len(idx))
            key.ck.append((basis, None, len(idx)))
            sig, _ = ecc.ScalePoints(ctx, cid, G1, basis, scalar=sigmas[ci], n=len(idx), out_device=True)
            key.ck[-1] = (basis, sig, len(idx))
        for name, group, k in (("alpha1", G1, alpha), ("beta1", G1, beta), ("delta1", G1, delta), ("beta2", G2, beta), ("delta2", G2, delta),
                               ("gamma2", G2, gamma)):
            key.points[name] = ecc.BatchScalarMultiplication(ctx, cid, group, gens[group], _elements(cid, [k], False))[0]
        if keep_scalars:
            key.scalars = {"A": tmp.pop("a"), "B": tmp.pop("b"), "Z": tmp.pop("z"), "K": tmp.pop("g0"), "vkK": tmp.pop("g1")}
            for ci in range(len(ck_idx)):
                key.scalars["CK%d" % ci] = tmp.pop("g%d" % (2 + ci))
        return key
    except Exception:
        key.free()
        raise
    finally:
        for b in tmp.values():
            b.free()


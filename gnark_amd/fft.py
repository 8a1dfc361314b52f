"""Mirror of gnark-crypto's `fft.Domain` as the reference uses it (backend/groth16/bn254/setup.go:101,
prove.go:346-389): `NewDomain(n)`, `FFT(a, DIF|DIT, on_coset)`, `FFTInverse(...)`, plus `compute_h`."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .device import Context, DeviceBuffer, _ptr, as_u64, curve_id

DIF, DIT = _lib.DIF, _lib.DIT


class Domain:
    def __init__(self, ctx: Context, curve, cardinality: int):
        """fft.NewDomain(m): cardinality is rounded up to the next power of two, as gnark-crypto does (at most 2^28 for BN254, 2^32 for
        BLS12-381, 2^47 for BLS12-377: the 2-adicity of r - 1)."""
        n = 1
        while n < cardinality:
            n *= 2
        self.ctx, self.curve, self.Cardinality = ctx, curve_id(curve), n
        h = C.c_void_p()
        ctx.lib.check(ctx.lib.ga_domain_create(ctx.handle, self.curve, n, C.byref(h)))
        self.handle = h

    def close(self):
        if self.handle:
            self.ctx.lib.ga_domain_destroy(self.handle)
            self.handle = None

    def _run(self, a, direction, decimation, on_coset):
        if isinstance(a, DeviceBuffer):
            self.ctx.lib.check(self.ctx.lib.ga_fft(self.handle, C.c_void_p(a.ptr), direction, decimation, int(on_coset), 1))
            return a
        a = as_u64(a, 4)
        if a.shape[0] != self.Cardinality:
            raise ValueError(f"len(a)={a.shape[0]} != domain cardinality {self.Cardinality}")
        out = a.copy()
        self.ctx.lib.check(self.ctx.lib.ga_fft(self.handle, _ptr(out), direction, decimation, int(on_coset), 0))
        return out

    def FFT(self, a, decimation: int, on_coset: bool = False):
        return self._run(a, _lib.FFT_FORWARD, decimation, on_coset)

    def FFTInverse(self, a, decimation: int, on_coset: bool = False):
        return self._run(a, _lib.FFT_INVERSE, decimation, on_coset)

    def _run_batch(self, a2d, direction, decimation, on_coset, count):
        n = self.Cardinality
        if isinstance(a2d, DeviceBuffer):
            if count is None:
                count = a2d.nbytes // (n * 32)
            if count * n * 32 > a2d.nbytes:
                raise ValueError(f"{count} vectors of {n} elements do not fit a device buffer of {a2d.nbytes} bytes")
            self.ctx.lib.check(self.ctx.lib.ga_fft_batch(self.handle, C.c_void_p(a2d.ptr), count, direction, decimation, int(on_coset), 1))
            return a2d
        a = np.ascontiguousarray(a2d, dtype=np.uint64)
        if a.ndim != 3 or a.shape[1:] != (n, 4) or (count is not None and count != a.shape[0]):
            raise ValueError(f"expected a (count, {n}, 4) uint64 array, got shape {a.shape}")
        out = a.copy()
        self.ctx.lib.check(self.ctx.lib.ga_fft_batch(self.handle, _ptr(out), out.shape[0], direction, decimation, int(on_coset), 0))
        return out

    def FFTBatch(self, a2d, decimation: int, on_coset: bool = False, count=None):
        """FFT of every vector of a2d, a (count, Cardinality, 4) array or a DeviceBuffer of `count` contiguous vectors (default: as many
        as the buffer holds), in one call: every pass of the transform is one launch over all of them (ga_fft_batch)."""
        return self._run_batch(a2d, _lib.FFT_FORWARD, decimation, on_coset, count)

    def FFTInverseBatch(self, a2d, decimation: int, on_coset: bool = False, count=None):
        return self._run_batch(a2d, _lib.FFT_INVERSE, decimation, on_coset, count)

    def compute_h_batch(self, A, B, C_) -> np.ndarray:
        """computeH for every solution of a batch (ga_compute_h_batch): A, B, C_ are (count, #constraints, 4) arrays; returns the
        (count, Cardinality, 4) array of the h vectors, each as compute_h's for its triple."""
        A, B, C_ = (np.ascontiguousarray(v, dtype=np.uint64) for v in (A, B, C_))
        if A.ndim != 3 or A.shape[2] != 4 or not (A.shape == B.shape == C_.shape):
            raise ValueError("A, B, C must be (count, n_constraints, 4) uint64 arrays of one shape")
        out = np.zeros((A.shape[0], self.Cardinality, 4), dtype=np.uint64)
        self.ctx.lib.check(self.ctx.lib.ga_compute_h_batch(self.handle, _ptr(A), _ptr(B), _ptr(C_), A.shape[0], A.shape[1], _ptr(out), 0))
        return out

    def compute_h(self, a, b, c) -> np.ndarray:
        """computeH (prove.go:346-389): a, b, c are the solver's A, B, C (len = #constraints <= n)."""
        a, b, c = as_u64(a, 4), as_u64(b, 4), as_u64(c, 4)
        if not (a.shape == b.shape == c.shape):
            raise ValueError("a, b, c must have the same length")
        out = np.zeros((self.Cardinality, 4), dtype=np.uint64)
        self.ctx.lib.check(self.ctx.lib.ga_compute_h(self.handle, _ptr(a), _ptr(b), _ptr(c), a.shape[0], _ptr(out), 0))
        return out


def NewDomain(ctx: Context, curve, m: int) -> Domain:
    return Domain(ctx, curve, m)

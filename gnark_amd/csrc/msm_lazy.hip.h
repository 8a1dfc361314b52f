// General-point arithmetic in the lazy (unreduced 29 / 28-bit limb) representation of field29.hip.h, shared by the window reduction
// (msm_reduce.hip.h: running sums, tree sums) and the window-table build (msm_bucket.hip.h: doubling chains).
#pragma once
#include "common.hip.h"
#include "field29.hip.h"

namespace ga {

template <class F> struct BaseFieldOf;
template <class Pp> struct BaseFieldOf<Fe<Pp>> { typedef Pp P; static constexpr bool IS_FP = true; };
template <class Pp> struct BaseFieldOf<Fe2<Pp>> { typedef Pp P; static constexpr bool IS_FP = false; };

// 64-lane tree reduction through LDS; result valid in lane 0
template <class F>
__device__ __forceinline__ XYZZ<F> wave_tree_sum(XYZZ<F> acc, XYZZ<F>* sh) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t stride = 32; stride >= 1; stride >>= 1) {
        sh[lane] = acc;
        __syncthreads();
        if (lane < stride) acc = add(acc, sh[lane + stride]);
        __syncthreads();
    }
    return acc;
}

// General XYZZ + XYZZ addition (add-2008-s) on unreduced limbs: 14 limb products with 13 reductions (Y3 fused), no modular
// corrections.  Exceptional inputs (equal or opposite points) are NOT handled: they make ZZ3 = 0 (mod p), which sticks to every
// later sum, so the caller tests ZZ once at the end and falls back to the exact arithmetic.  Constants: tools/lazy_bounds.py
// check_add.
template <class F>
struct Lazy4 {
    typename Lazy<F>::T x, y, zz, zzz;
};
template <class F>
__device__ __forceinline__ Lazy4<F> lazy4_from_mem(const XYZZ<F>& p) {
    return {Lazy<F>::from_mem(p.x), Lazy<F>::from_mem(p.y), Lazy<F>::from_mem(p.zz), Lazy<F>::from_mem(p.zzz)};
}
template <class F>
__device__ __forceinline__ void add29(Lazy4<F>& a, const Lazy4<F>& b) {
    typedef typename Lazy<F>::T T;
    typedef typename Lazy<F>::Params P;
    constexpr int KMS = Lazy<F>::FP2 ? P::FP2Z_K : 8;
    T U1 = f29_mul(a.x, b.zz);
    T U2 = f29_mul(b.x, a.zz);
    T S1 = f29_mul(a.y, b.zzz);
    T S2 = f29_mul(b.y, a.zzz);
    T Pp = f29_sub<4>(U2, U1);
    T R = f29_sub<4>(S2, S1);
    T PP = f29_sqr(Pp);
    T PPP = f29_mul(Pp, PP);
    T Q = f29_mul(U1, PP);
    T X3 = f29_sub<4>(f29_sqr(R), f29_add(PPP, f29_add(Q, Q)));
    if constexpr (Lazy<F>::FP2) X3 = f29_partial_reduce(X3);
    a.y = f29_mul_sub<KMS>(R, f29_sub<8>(Q, X3), S1, PPP);
    a.x = X3;
    a.zz = f29_mul(f29_mul(a.zz, b.zz), PP);
    a.zzz = f29_mul(f29_mul(a.zzz, b.zzz), PPP);
}

// 2 P for a general XYZZ point in the lazy representation (dbl-2008-s-1, a = 0); bounds: tools/lazy_bounds.py check_dbl (the fixed
// point of repeated doublings, the same subtraction constants as mdbl29)
template <class F>
__device__ __forceinline__ void dbl29(Lazy4<F>& a) {
    typedef typename Lazy<F>::T T;
    typedef typename Lazy<F>::Params P;
    constexpr int KMS = Lazy<F>::FP2 ? P::FP2Z_K : 8;
    const T U = f29_add(a.y, a.y);
    const T V = f29_sqr(U);
    const T W = f29_mul(U, V);
    const T S = f29_mul(a.x, V);
    const T xx = f29_sqr(a.x);
    const T M = f29_add(f29_add(xx, xx), xx);
    T X3 = f29_sub<4>(f29_sqr(M), f29_add(S, S));
    if constexpr (Lazy<F>::FP2) X3 = f29_partial_reduce(X3);
    const T Y3 = f29_mul_sub<KMS>(M, f29_sub<8>(S, X3), W, a.y);
    a.zz = f29_mul(V, a.zz);
    a.zzz = f29_mul(W, a.zzz);
    a.x = X3;
    a.y = Y3;
}

// ---- block-wide sums of XYZZ points in the lazy representation ---------------------------------------------------------------
// The tree sums after the group pass (per-bit sums, segment sums) are LATENCY-bound: one wave per block adds a handful of points
// serially and then walks a 6-level tree, every step an addition in the exact packed arithmetic (~20 us G1, ~60 us G2 per dependent
// addition).  In the lazy representation a dependent addition is ~3x shorter.  Exceptional additions (equal or opposite points: never
// for sums of distinct random buckets, always for a degenerate key) leave ZZ == 0; the block then repeats its sum exactly.
template <class F>
struct LazyPt {
    Lazy4<F> v;
    uint32_t inf;
};
template <class F>
__device__ __forceinline__ void lazy_acc(LazyPt<F>& acc, const XYZZ<F>& p) {
    if (is_inf(p)) return;
    const Lazy4<F> b = lazy4_from_mem<F>(p);
    if (acc.inf) {
        acc.v = b;
        acc.inf = 0;
    } else {
        add29<F>(acc.v, b);
    }
}
template <class F>
__device__ __forceinline__ void lazy_acc(LazyPt<F>& acc, const LazyPt<F>& b) {
    if (b.inf) return;
    if (acc.inf) acc = b;
    else add29<F>(acc.v, b.v);
}
// sum over the block's 64 lanes (result in lane 0) of the points src(i), i = lane, lane + 64, ... < count; written to *dst.
// src(i) returns a pointer to the i-th input of this block.
template <class F, class Src>
__device__ __forceinline__ void block_sum29(uint32_t count, Src src, XYZZ<F>* dst, LazyPt<F>* sh, XYZZ<F>* shx, uint32_t* bad) {
    const uint32_t lane = threadIdx.x;
    LazyPt<F> acc;
    acc.inf = 1;
    for (uint32_t i = lane; i < count; i += 64) lazy_acc<F>(acc, load_pod<XYZZ<F>>(src(i)));
    for (uint32_t stride = 32; stride >= 1; stride >>= 1) {
        sh[lane] = acc;
        __syncthreads();
        if (lane < stride) lazy_acc<F>(acc, sh[lane + stride]);
        __syncthreads();
    }
    if (lane == 0) {
        XYZZ<F> out = xyzz_inf<F>();
        uint32_t b = 0;
        if (!acc.inf) {
            out.zz = Lazy<F>::to_mem(acc.v.zz);
            b = is_zero(out.zz) ? 1u : 0u;
            out.x = Lazy<F>::to_mem(acc.v.x);
            out.y = Lazy<F>::to_mem(acc.v.y);
            out.zzz = Lazy<F>::to_mem(acc.v.zzz);
        }
        if (!b) store_pod(dst, out);
        *bad = b;
    }
    __syncthreads();
    if (*bad) {   // an exceptional addition somewhere in this block's sum: once more with the complete formulas
        XYZZ<F> e = xyzz_inf<F>();
        for (uint32_t i = lane; i < count; i += 64) e = add(e, load_pod<XYZZ<F>>(src(i)));
        e = wave_tree_sum(e, shx);
        if (lane == 0) store_pod(dst, e);
    }
    __syncthreads();
}

}  // namespace ga

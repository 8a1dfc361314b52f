// Host-side group helpers used by the proof epilogue (prove.go:185,199-200,212-214,241-269,287-292) and by the
// multi-GPU combine.  Same templates as the device code, compiled for the host: a handful of scalar
// multiplications and additions per proof, which the reference also keeps on the CPU
// (icicle.go:1096-1097,1144-1146,1249-1259,1309-1314).
#pragma once
#include "common.hip.h"

namespace ga {

template <class F>
inline XYZZ<F> host_load_jac(const void* p) {
    Jac<F> j;
    memcpy(&j, p, sizeof(j));
    return from_jac(j);
}
template <class F>
inline void host_store_jac(void* p, const XYZZ<F>& a) {
    Jac<F> j = to_jac(a);
    memcpy(p, &j, sizeof(j));
}
template <class F>
inline XYZZ<F> host_load_affine(const void* p) {
    Affine<F> a;
    memcpy(&a, p, sizeof(a));
    return to_xyzz(a);
}
template <class F>
inline void host_store_affine(void* p, const XYZZ<F>& a) {
    Affine<F> r = to_affine(a);
    memcpy(p, &r, sizeof(r));
}

// scalar: fr element in Montgomery form -> canonical 8 words
template <class FrP>
inline void host_fr_canonical(const void* fr_mont, uint32_t* out8) {
    Fe<FrP> s;
    memcpy(s.l, fr_mont, 32);
    s = from_mont(s);
    memcpy(out8, s.l, 32);
}

// result = sum_j 2^(c*j) W_j  (host; Horner from the top window)
template <class F>
XYZZ<F> host_horner(const XYZZ<F>* W, int nwin, int c) {
    XYZZ<F> acc = xyzz_inf<F>();
    for (int w = nwin - 1; w >= 0; w--) {
        for (int k = 0; k < c; k++) acc = dbl(acc);
        acc = add(acc, W[w]);
    }
    return acc;
}

// the host group helpers of the C ABI (ga_jac_add, ga_jac_to_affine, ga_jac_scalar_mul / ga_generator_mul, ga_msm_combine_windows):
// Jac<F> images in and out, k = 8 canonical words
template <class F>
inline void host_jac_add(const void* a, const void* b, void* out) {
    host_store_jac<F>(out, add(host_load_jac<F>(a), host_load_jac<F>(b)));
}
template <class F>
inline void host_jac_to_affine(const void* a, void* out) {
    host_store_affine<F>(out, host_load_jac<F>(a));
}
template <class F>
inline void host_jac_scalar_mul(const XYZZ<F>& a, const void* k, void* out) {
    uint32_t kw[8];
    memcpy(kw, k, 32);
    host_store_jac<F>(out, scalar_mul(a, kw, 8));
}
template <class F>
inline void host_jac_horner(const void* windows, int nwin, int c, void* out) {
    std::vector<XYZZ<F>> W(nwin);
    for (int w = 0; w < nwin; w++) W[w] = host_load_jac<F>(reinterpret_cast<const char*>(windows) + (size_t)w * sizeof(Jac<F>));
    host_store_jac<F>(out, host_horner(W.data(), nwin, c));
}

// contiguous share `index` of `count` of nwin windows (same split as multigpu.shard_range)
inline void window_share(int nwin, uint32_t index, uint32_t count, int* lo, int* hi) {
    const int base = nwin / (int)count, rem = nwin % (int)count, k = (int)index;
    *lo = k * base + (k < rem ? k : rem);
    *hi = *lo + base + (k < rem ? 1 : 0);
}

// An MSM over raw bases on the device -> XYZZ: msm_run (msm.hip.h) over the planned window width and share (win_index, win_count) of
// the windows (multi-GPU partition A): the other windows count as zero in the Horner sum, so shares add up.
template <class C, int G>
int host_msm(Ctx* ctx, const void* d_bases, const void* d_scalars, size_t n, bool mont,
             XYZZ<typename GroupField<C, G>::F>* out, uint32_t win_index = 0, uint32_t win_count = 1) {
    int c, nwin, lo, hi;
    GA_CHECK(msm_plan<C>(G, n, &c, &nwin));
    window_share(nwin, win_index, win_count ? win_count : 1, &lo, &hi);
    *out = xyzz_inf<typename GroupField<C, G>::F>();
    if (hi <= lo) return GA_OK;   // an empty share
    return msm_run<C, G>(ctx, d_bases, d_scalars, n, mont, c, lo, hi, (size_t)ctx->tun.msm_max_chunk, out, false);
}

}  // namespace ga

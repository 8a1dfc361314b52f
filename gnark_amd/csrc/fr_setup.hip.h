// The three small Fr vector calls around fr_sparse.hip.h that keep the scalar side of groth16.Setup on the device:
//   fr_lagrange_run   out[i] = L_i(tau), i < m: the Lagrange basis of the size-n domain at one point (setup.go:356-421 computes it with a
//                     running product and one fr.BatchInvert).  L_i = (tau^n - 1) / n * w^i * inv(tau - w^i), inv(0) = 0:
//                       fr_lagrange_points_kernel   w^i into `out` and tau - w^i into scratch: a workgroup covers 256 * 16 consecutive indices,
//                                                   lane l starts at w^(base + l) (pow_u64) and steps by w^256, so every store is coalesced;
//                       fr_batch_inverse            the device batch inversion of plonk.hip.h, zeros stay zero;
//                       fr_lagrange_fuse_kernel     out[i] = c * out[i] * inv[i], c = (tau^n - 1) / n from the host, in the output form.
//   fr_compact_run    the zero filter of setup.go:195-219: flags, hipcub::DeviceScan::ExclusiveSum, scatter.
//   fr_powers_run     out[i] = c * t^(first + i) (setup.go:181-192; kzg.NewSRS): fr_power_term of fr_powers.hip.h, one term per lane.
#pragma once
#include <hipcub/hipcub.hpp>

#include <vector>

#include "fr_powers.hip.h"
#include "vec_call.hip.h"   // StreamDrain, chunk_in / chunk_out

namespace ga {

constexpr unsigned FR_LAGRANGE_RUN = 16;   // powers per lane: one pow_u64 (about 1.5 log2 n products) is shared by 16 elements

template <class FrP>
__global__ void __launch_bounds__(256)
fr_lagrange_points_kernel(const Fe<FrP> w, const Fe<FrP> wstep, const Fe<FrP> tau, uint64_t m, uint32_t* __restrict__ pw, uint32_t* __restrict__ den) {
    const uint64_t base = (uint64_t)blockIdx.x * (256 * FR_LAGRANGE_RUN) + threadIdx.x;
    if (base >= m) return;
    Fe<FrP> p = pow_u64(w, base);
#pragma unroll 1
    for (uint32_t k = 0; k < FR_LAGRANGE_RUN; k++) {
        const uint64_t i = base + (uint64_t)k * 256;
        if (i >= m) break;
        store_pod(pw + i * 8, p);
        store_pod(den + i * 8, sub(tau, p));
        p = mul(p, wstep);
    }
}

template <class FrP>
__global__ void __launch_bounds__(256)
fr_lagrange_fuse_kernel(const Fe<FrP> c, const uint32_t* __restrict__ inv_den, uint64_t m, int mont, uint32_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    Fe<FrP> v = mul(mul(c, load_pod<Fe<FrP>>(out + i * 8)), load_pod<Fe<FrP>>(inv_den + i * 8));
    if (!mont) v = from_mont(v);
    store_pod(out + i * 8, v);
}

// one host element as the ABI takes it -> Montgomery, below r
template <class FrP>
inline Fe<FrP> fr_host_element(const void* p, bool mont) {
    Fe<FrP> e;
    memcpy(&e, p, 32);
    return mont ? e : to_mont(fr_canonical(e, 0));
}

// n = 2^logn, m <= n (validated by the entry point)
template <class C>
int fr_lagrange_run(Ctx* ctx, int logn, const void* tau, size_t m, unsigned flags, void* out) {
    typedef typename C::FrP FrP;
    typedef Fe<FrP> F;
    const bool mont = (flags & GA_SCALARS_MONTGOMERY) != 0, o_dev = (flags & GA_RESULT_ON_DEVICE) != 0;
    const F t = fr_host_element<FrP>(tau, mont);
    F w = fe_const<FrP>(FrP::ROOT);   // the generator fft.NewDomain(n) takes: ROOT^(2^(adicity - logn))
    for (int k = 0; k < FrP::ADICITY - logn; k++) w = sqr(w);
    const F wstep = pow_u64(w, 256);
    F tn = t, nf = fe_zero<FrP>();
    for (int k = 0; k < logn; k++) tn = sqr(tn);
    nf.l[0] = (uint32_t)(1ull << logn);
    nf.l[1] = (uint32_t)((1ull << logn) >> 32);
    const F c = mul(sub(tn, fe_one<FrP>()), inv(to_mont(nf)));
    hipStream_t st = ctx->work_stream();
    uint32_t *den, *d_out = nullptr;
    GA_CHECK(ctx->scratch_get("fr_lagrange_den", m * 32, (void**)&den));
    if (!o_dev) GA_CHECK(ctx->scratch_get("fr_lagrange_out", m * 32, (void**)&d_out));
    uint32_t* dst = o_dev ? (uint32_t*)out : d_out;
    StreamDrain drain{st};
    {
        StageTimer tm(ctx, "fr_lagrange_points");
        const uint64_t per = 256 * FR_LAGRANGE_RUN;
        hipLaunchKernelGGL((fr_lagrange_points_kernel<FrP>), dim3((unsigned)((m + per - 1) / per)), dim3(256), 0, st, w, wstep, t, (uint64_t)m, dst, den);
        GA_KERNEL_CHECK();
    }
    // (fr_batch_inverse launches on ctx->stream: the same stream as work_stream() here, because an ABI call under CtxLock runs on lane 0;
    //  it also synchronises that stream before it returns)
    GA_CHECK(fr_vec_batch_inverse<C>(ctx, den, m, true));
    {
        StageTimer tm(ctx, "fr_lagrange_fuse");
        hipLaunchKernelGGL((fr_lagrange_fuse_kernel<FrP>), dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, c, (const uint32_t*)den, (uint64_t)m, (int)mont, dst);
        GA_KERNEL_CHECK();
    }
    GA_CHECK(chunk_out(st, o_dev, (uint32_t*)out, 0, m * 8, d_out));
    GA_HIP_CHECK(hipStreamSynchronize(st));
    return GA_OK;
}

// ---- the zero filter ---------------------------------------------------------------------------------------------------------------
template <class FrP>
__global__ void __launch_bounds__(256)
fr_nonzero_flag_kernel(const uint32_t* __restrict__ v, uint32_t n, uint32_t* __restrict__ keep, uint8_t* __restrict__ mask) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool zero = is_zero(load_pod<Fe<FrP>>(v + (uint64_t)i * 8));
    keep[i] = zero ? 0u : 1u;
    if (mask) mask[i] = zero ? 1 : 0;
}

template <class FrP>
__global__ void __launch_bounds__(256)
fr_compact_scatter_kernel(const uint32_t* __restrict__ v, uint32_t n, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ off,
                          uint32_t* __restrict__ dst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !keep[i]) return;
    store_pod(dst + (uint64_t)off[i] * 8, load_pod<Fe<FrP>>(v + (uint64_t)i * 8));   // off[i] <= i < n
}

// 1 <= n <= 2^31 - 1 (validated by the entry point)
template <class C>
int fr_compact_run(Ctx* ctx, const void* v, size_t n, unsigned flags, void* out, uint8_t* mask, uint64_t* count) {
    typedef typename C::FrP FrP;
    const bool i_dev = (flags & GA_BASES_ON_DEVICE) != 0, o_dev = (flags & GA_RESULT_ON_DEVICE) != 0;
    const bool direct = o_dev && !(i_dev && out == v);   // the scatter may write `out` itself; in place it goes through scratch
    hipStream_t st = ctx->work_stream();
    size_t tmp_bytes = 0;
    GA_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, st));
    uint32_t *keep, *off, *d_v = nullptr, *d_dst = nullptr;
    uint8_t* d_mask = nullptr;
    void* tmp;
    GA_CHECK(ctx->scratch_get("fr_compact_keep", n * 4, (void**)&keep));
    GA_CHECK(ctx->scratch_get("fr_compact_offsets", n * 4, (void**)&off));
    GA_CHECK(ctx->scratch_get("fr_compact_scan", tmp_bytes, &tmp));
    if (mask) GA_CHECK(ctx->scratch_get("fr_compact_mask", n, (void**)&d_mask));
    if (!i_dev) GA_CHECK(ctx->scratch_get("fr_compact_in", n * 32, (void**)&d_v));
    if (!direct) GA_CHECK(ctx->scratch_get("fr_compact_out", n * 32, (void**)&d_dst));
    StreamDrain drain{st};
    const uint32_t* src;
    GA_CHECK(chunk_in(st, i_dev, (const uint32_t*)v, 0, n * 8, d_v, &src));
    uint32_t* dst = direct ? (uint32_t*)out : d_dst;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    uint32_t tail[2] = {0, 0};   // the last offset and the last flag: their sum is the number kept
    {
        StageTimer tm(ctx, "fr_compact");
        hipLaunchKernelGGL((fr_nonzero_flag_kernel<FrP>), dim3(blocks), dim3(256), 0, st, src, (uint32_t)n, keep, d_mask);
        GA_KERNEL_CHECK();
        GA_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, (const uint32_t*)keep, off, (int)n, st));
        hipLaunchKernelGGL((fr_compact_scatter_kernel<FrP>), dim3(blocks), dim3(256), 0, st, src, (uint32_t)n, (const uint32_t*)keep, (const uint32_t*)off, dst);
        GA_KERNEL_CHECK();
    }
    GA_HIP_CHECK(hipMemcpyAsync(&tail[0], off + (n - 1), 4, hipMemcpyDeviceToHost, st));
    GA_HIP_CHECK(hipMemcpyAsync(&tail[1], keep + (n - 1), 4, hipMemcpyDeviceToHost, st));
    if (mask) GA_HIP_CHECK(hipMemcpyAsync(mask, d_mask, n, hipMemcpyDeviceToHost, st));
    GA_HIP_CHECK(hipStreamSynchronize(st));
    const uint64_t kept = (uint64_t)tail[0] + tail[1];
    if (!direct && kept) {
        GA_HIP_CHECK(hipMemcpyAsync(out, d_dst, kept * 32, o_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
        GA_HIP_CHECK(hipStreamSynchronize(st));
    }
    *count = kept;
    return GA_OK;
}

// ---- powers --------------------------------------------------------------------------------------------------------------------------
template <class FrP>
__global__ void __launch_bounds__(256)
fr_powers_kernel(const Fe<FrP> c, const Fe<FrP> t, int mont, uint64_t first, uint64_t n, uint32_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fe<FrP> s = fr_power_term(c, t, mont, first + i);
    if (mont) s = to_mont(s);
    store_pod(out + i * 8, s);
}

// 1 <= n <= 2^32 (validated by the entry point); scalars: (c, t) on the host
template <class C>
int fr_powers_run(Ctx* ctx, const void* scalars, uint64_t first, size_t n, unsigned flags, void* out) {
    typedef typename C::FrP FrP;
    const bool mont = (flags & GA_SCALARS_MONTGOMERY) != 0, o_dev = (flags & GA_RESULT_ON_DEVICE) != 0;
    Fe<FrP> c, t;
    memcpy(&c, scalars, 32);
    memcpy(&t, (const char*)scalars + 32, 32);
    hipStream_t st = ctx->work_stream();
    uint32_t* d_out = nullptr;
    if (!o_dev) GA_CHECK(ctx->scratch_get("fr_powers_out", n * 32, (void**)&d_out));
    StreamDrain drain{st};
    {
        StageTimer tm(ctx, "fr_powers");
        hipLaunchKernelGGL((fr_powers_kernel<FrP>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, c, t, (int)mont, first, (uint64_t)n, o_dev ? (uint32_t*)out : d_out);
        GA_KERNEL_CHECK();
    }
    GA_CHECK(chunk_out(st, o_dev, (uint32_t*)out, 0, n * 8, d_out));
    GA_HIP_CHECK(hipStreamSynchronize(st));
    return GA_OK;
}

// what fr_setup_<curve>.hip instantiates, with GA_INSTANTIATE_FR_SPARSE (fr_sparse.hip.h)
#define GA_INSTANTIATE_FR_SETUP(C)                                                                   \
    template int fr_lagrange_run<C>(Ctx*, int, const void*, size_t, unsigned, void*);                \
    template int fr_compact_run<C>(Ctx*, const void*, size_t, unsigned, void*, uint8_t*, uint64_t*); \
    template int fr_powers_run<C>(Ctx*, const void*, uint64_t, size_t, unsigned, void*);

}  // namespace ga

// kzg.ToLagrangeG1 (gnark-crypto ecc/<curve>/kzg) and mpcsetup's lagrangeCoeffsG1 / lagrangeCoeffsG2 (backend/groth16/<curve>/mpcsetup/
// lagrange.go:21-64): the inverse FFT whose elements are points of G1 or G2 (ec_ntt_to_lagrange<C, G>; F = GroupField<C, G>::F).
//     out[i] = [1/n] sum_j [w^(-i j)] powers[j],   w = the generator of the size-n domain (fft.NewDomain(n)), natural order in and out
// -- n/2 log2 n full-width variable-base scalar multiplications, the whole cost of turning a ceremony SRS into its Lagrange form.
//
// On the context's work stream, one host synchronisation (device-resident input and output):
//   1. ec_ntt_twiddle_kernel   tw[j] = w^(-j), j < n/2, as canonical scalars; stage s reads them with stride 2^s.
//   2. ec_ntt_load_kernel      affine input -> the work array: XYZZ points whose coordinates are canonical packed hat-domain words
//                              (the format of fixed_base.hip.h's sums), all-zero = infinity.  The input is never written.
//   3. ec_ntt_stage_kernel     log2 n radix-2 DIF stages in place, one lane per butterfly (a, b) -> (a + b, [k](a - b)) with
//                              k = w^(-j 2^s).  Both additions are add29 and the multiplication is left-to-right double-and-add on
//                              dbl29 / add29 (msm_lazy.hip.h), the accumulator in registers and the base a - b in the lane's LDS
//                              column.  Nothing is branched on inside the loop: a = +-b, a point of small order, a doubling of a
//                              2-torsion point all end in ZZ == 0 (mod p), which is absorbing, so ONE exact test of the two results
//                              flags the lane; a lane with an operand at infinity is flagged before it starts.  Flagged butterflies
//                              are left untouched and redone by ec_ntt_exact_kernel with the complete formulas of ec.hip.h.
//                              k = 1 (j = 0; the whole last stage) skips the multiplication.
//                              The factor 1/n rides on the twiddles of group 0 of every stage (k = w^(-j 2^s) / n there): an element
//                              takes its first b-branch out of group 0, so after the last stage every element but the one at
//                              position 0 carries 1/n exactly once, at the price of log2 n extra multiplications (the j = 0 lanes of
//                              group 0).  ec_ntt_scale_kernel multiplies position 0.
//                              Lane order: from stage 6 on (2^s >= 64 groups) the lanes of a wave are the SAME butterfly j of 64
//                              consecutive groups, so they share the scalar and the add-or-not branch of the loop is wave-uniform;
//                              before that a wave holds 64 consecutive j of one group and executes the addition for nearly every bit.
//   4. fixed_base_affine_kernel (fixed_base.hip.h)  XYZZ -> affine with one inversion per lane batch, written at the bit-reversed
//                              index: the DIF stages leave the result in bit-reversed order.
#pragma once
#include "fixed_base.hip.h"   // fixed_base_affine_kernel; Table29, LdsAcc29 (msm_bucket.hip.h); add29, dbl29 (msm_lazy.hip.h); vec_call.hip.h

namespace ga {

// waves per SIMD asked of the stage kernel: 175 VGPRs for the 9-limb field either way; the 14-limb field takes 269 without the bound
// (one wave per SIMD) and 256 with 15 spilled registers under it -- two workgroups of 68 KiB of LDS then fit a CU
constexpr int EC_NTT_MIN_WAVES = 2;
constexpr unsigned EC_NTT_EXACT_MAX_BLOCKS = 1024;   // one-wave workgroups of the exact redo (its private segment is per resident wave)
// over Fp2 one extended point is 72 (BN254) or 112 (BLS12-381) registers and the butterfly holds two around the ladder: under the
// two-wave bound the BN254 G2 kernel spilled 250 registers (688 B of scratch per lane), with the whole register file of a SIMD lane
// it spills 11 and the transform runs 10 % faster at 2^12 and 2^16, 3 % at 2^18 (same box, G1 unchanged beside it).
// BLS12-381 G2 runs 128-lane workgroups, for which both bounds mean one wave per SIMD.  G1 keeps EC_NTT_MIN_WAVES
template <class F> struct EcNttStage {
    static constexpr int MIN_WAVES = Lazy<F>::FP2 ? 1 : EC_NTT_MIN_WAVES;
};

template <class FrP>
__global__ void __launch_bounds__(256)
ec_ntt_twiddle_kernel(uint32_t* __restrict__ tw, uint64_t half, const Fe<FrP> winv) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= half) return;
    store_pod(tw + j * 8, from_mont(pow_u64(winv, j)));
}

template <class F>
__global__ void __launch_bounds__(256)
ec_ntt_load_kernel(const Affine<F>* __restrict__ in, uint64_t n, XYZZ<F>* __restrict__ work) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Affine<F> a = load_pod<Affine<F>>(&in[i]);
    const F z = FieldTraits<F>::zero();
    XYZZ<F> o{z, z, z, z};
    if (!is_inf(a)) {
        const F one = Lazy<F>::hat_packed(FieldTraits<F>::one());
        o = {Lazy<F>::hat_packed(a.x), Lazy<F>::hat_packed(a.y), one, one};
    }
    store_pod(&work[i], o);
}

// butterfly t of stage s: its two positions and its scalar (canonical words); returns false when the scalar is 1
struct EcNttButterfly {
    uint64_t ia, ib;
    uint32_t k[8];
};
template <class FrP>
__device__ __forceinline__ bool ec_ntt_butterfly(uint64_t t, int s, int logn, int uniform, const uint32_t* __restrict__ tw, const Fe<FrP>& ninv_mont,
                                                 EcNttButterfly& B) {
    const int lm = logn - 1 - s;   // log2 of the butterflies per group
    uint64_t g, j;
    if (uniform && s >= 6) {
        j = t >> s;
        g = t & ((1ull << s) - 1);
    } else {
        g = t >> lm;
        j = t & ((1ull << lm) - 1);
    }
    B.ia = (g << (lm + 1)) + j;
    B.ib = B.ia + (1ull << lm);
    if (g != 0 && j == 0) return false;
    Fe<FrP> k = load_pod<Fe<FrP>>(tw + (j << s) * 8);
    if (g == 0) k = mul(k, ninv_mont);   // canonical * Montgomery -> canonical: w^(-j 2^s) / n
#pragma unroll
    for (int i = 0; i < 8; i++) B.k[i] = k.l[i];
    return true;
}

__device__ __forceinline__ int ec_ntt_top_bit(const uint32_t (&k)[8]) {
    int top = -1;
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (k[i]) top = 32 * i + 31 - __clz(k[i]);
    return top;
}

// acc = [k] acc for k >= 1 in the lazy representation: the base is parked in the lane's LDS column, the accumulator stays in
// registers; one doubling per bit below the top one and one general addition per set bit.  Bounds: tools/lazy_bounds.py check_ladder.
template <class F>
__device__ __forceinline__ void ec_ntt_scalar_mul29(Lazy4<F>& acc, const LdsAcc29<F>& D, const uint32_t (&k)[8]) {
    D.put(0, acc.x);
    D.put(1, acc.y);
    D.put(2, acc.zz);
    D.put(3, acc.zzz);
    for (int b = ec_ntt_top_bit(k) - 1; b >= 0; b--) {
        dbl29<F>(acc);
        if ((k[b >> 5] >> (b & 31)) & 1) {
            const Lazy4<F> d{D.get(0), D.get(1), D.get(2), D.get(3)};
            add29<F>(acc, d);
        }
    }
}

template <class F>
__device__ __forceinline__ Lazy4<F> ec_ntt_unpack(const XYZZ<F>& p) {
    return {Lazy<F>::unpack(p.x), Lazy<F>::unpack(p.y), Lazy<F>::unpack(p.zz), Lazy<F>::unpack(p.zzz)};
}
template <class F>
__device__ __forceinline__ XYZZ<F> ec_ntt_pack(const Lazy4<F>& p) {
    return {f29_pack_hat(p.x), f29_pack_hat(p.y), f29_pack_hat(p.zz), f29_pack_hat(p.zzz)};
}
// work-array point <-> the exact arithmetic's XYZZ (gnark's Montgomery image)
template <class F>
__device__ __forceinline__ XYZZ<F> ec_ntt_to_exact(const XYZZ<F>& p) {
    if (is_inf(p)) return xyzz_inf<F>();
    return {Lazy<F>::to_mem(Lazy<F>::unpack(p.x)), Lazy<F>::to_mem(Lazy<F>::unpack(p.y)), Lazy<F>::to_mem(Lazy<F>::unpack(p.zz)),
            Lazy<F>::to_mem(Lazy<F>::unpack(p.zzz))};
}
template <class F>
__device__ __forceinline__ XYZZ<F> ec_ntt_from_exact(const XYZZ<F>& p) {
    const F z = FieldTraits<F>::zero();
    if (is_inf(p)) return {z, z, z, z};
    return {Lazy<F>::hat_packed(p.x), Lazy<F>::hat_packed(p.y), Lazy<F>::hat_packed(p.zz), Lazy<F>::hat_packed(p.zzz)};
}
// an affine point that is not (0,0) -> the lazy representation, ZZ = ZZZ = 1
template <class F>
__device__ __forceinline__ Lazy4<F> affine_to_lazy4(const Affine<F>& a) {
    const typename Lazy<F>::T one = Lazy<F>::from_mem(FieldTraits<F>::one());
    return {Lazy<F>::from_mem(a.x), Lazy<F>::from_mem(a.y), one, one};
}

template <class F, class FrP>
__global__ void __launch_bounds__(Table29<F>::THREADS, EcNttStage<F>::MIN_WAVES)
ec_ntt_stage_kernel(XYZZ<F>* __restrict__ work, const uint32_t* __restrict__ tw, uint64_t half, int s, int logn, int uniform, const Fe<FrP> ninv_mont,
                    uint32_t* __restrict__ redo, uint32_t* __restrict__ redo_count) {
    constexpr int NW = Lazy<F>::NW;
    __shared__ uint32_t lds[4 * NW * Table29<F>::THREADS];
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= half) return;
    EcNttButterfly B;
    const bool scaled = ec_ntt_butterfly<FrP>(t, s, logn, uniform, tw, ninv_mont, B);
    const XYZZ<F> pa = load_pod<XYZZ<F>>(&work[B.ia]), pb = load_pod<XYZZ<F>>(&work[B.ib]);
    if (is_inf(pa) | is_inf(pb)) {
        redo[atomicAdd(redo_count, 1u)] = (uint32_t)t;
        return;
    }
    // a - b and its multiple first; a + b after the loop, from operands read again: nothing but the accumulator and the scalar
    // is live across the loop (the sum costs 14 of the butterfly's ~4000 products)
    Lazy4<F> diff = ec_ntt_unpack<F>(pa);
    {
        Lazy4<F> b = ec_ntt_unpack<F>(pb);
        b.y = f29_sub<2>(Lazy<F>::from_mem(FieldTraits<F>::zero()), b.y);   // 2p - y
        add29<F>(diff, b);
    }
    if (scaled) ec_ntt_scalar_mul29<F>(diff, LdsAcc29<F>(lds + threadIdx.x), B.k);
    Lazy4<F> sum = ec_ntt_unpack<F>(load_pod<XYZZ<F>>(&work[B.ia]));
    add29<F>(sum, ec_ntt_unpack<F>(load_pod<XYZZ<F>>(&work[B.ib])));
    if (f29_is_zero_mod_p(sum.zz) | f29_is_zero_mod_p(diff.zz)) {   // a flagged lane leaves a and b as they were
        redo[atomicAdd(redo_count, 1u)] = (uint32_t)t;
        return;
    }
    store_pod(&work[B.ia], ec_ntt_pack<F>(sum));
    store_pod(&work[B.ib], ec_ntt_pack<F>(diff));
}

// the flagged butterflies of a stage once more, with the complete formulas (grid-stride over the redo list)
template <class F, class FrP>
__global__ void __launch_bounds__(64)
ec_ntt_exact_kernel(XYZZ<F>* __restrict__ work, const uint32_t* __restrict__ tw, int s, int logn, int uniform, const Fe<FrP> ninv_mont,
                    const uint32_t* __restrict__ redo, const uint32_t* __restrict__ redo_count) {
    const uint32_t nredo = *redo_count;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < nredo; r += gridDim.x * blockDim.x) {
        EcNttButterfly B;
        const bool scaled = ec_ntt_butterfly<FrP>(redo[r], s, logn, uniform, tw, ninv_mont, B);
        const XYZZ<F> a = ec_ntt_to_exact<F>(load_pod<XYZZ<F>>(&work[B.ia])), b = ec_ntt_to_exact<F>(load_pod<XYZZ<F>>(&work[B.ib]));
        XYZZ<F> diff = add(a, neg(b));
        if (scaled) diff = scalar_mul(diff, B.k, 8);
        store_pod(&work[B.ia], ec_ntt_from_exact<F>(add(a, b)));
        store_pod(&work[B.ib], ec_ntt_from_exact<F>(diff));
    }
}

// work[i] = [k] work[i] for i < count (k a canonical scalar >= 1): the element the stages leave without its 1/n
template <class F, class FrP>
__global__ void __launch_bounds__(Table29<F>::THREADS)
ec_ntt_scale_kernel(XYZZ<F>* __restrict__ work, uint32_t count, const Fe<FrP> k_canonical) {
    constexpr int NW = Lazy<F>::NW;
    __shared__ uint32_t lds[4 * NW * Table29<F>::THREADS];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const XYZZ<F> p = load_pod<XYZZ<F>>(&work[i]);
    if (is_inf(p)) return;
    uint32_t k[8];
#pragma unroll
    for (int w = 0; w < 8; w++) k[w] = k_canonical.l[w];
    Lazy4<F> acc = ec_ntt_unpack<F>(p);
    LdsAcc29<F> D(lds + threadIdx.x);
    ec_ntt_scalar_mul29<F>(acc, D, k);
    if (f29_is_zero_mod_p(acc.zz))   // a point of small order: the complete formulas
        store_pod(&work[i], ec_ntt_from_exact<F>(scalar_mul(ec_ntt_to_exact<F>(p), k, 8)));
    else
        store_pod(&work[i], ec_ntt_pack<F>(acc));
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// uniform: the lane order of stages >= 6 (1: one scalar per wave, the default; 0: consecutive j, the A/B of tools/to_lagrange_bench.py)
template <class C, int G>
int ec_ntt_to_lagrange(Ctx* ctx, const void* powers, size_t n, unsigned flags, void* out, int uniform) {
    typedef typename GroupField<C, G>::F F;
    typedef typename C::FrP FrP;
    if ((n & (n - 1)) != 0 || ilog2_u64(n) > FrP::ADICITY) {
        set_error("%s: n = %zu is not a power of two up to 2^%d", current_entry(), n, (int)FrP::ADICITY);
        return GA_ERR_INVALID;
    }
    if ((uint64_t)n > (1ull << 31)) {   // (BLS12-381 admits 2^32: 768 GiB of work array; the kernels index butterflies with 32 bits)
        set_error("%s: n = %zu needs more device memory than there is", current_entry(), n);
        return GA_ERR_NOMEM;
    }
    const bool i_dev = (flags & GA_BASES_ON_DEVICE) != 0, o_dev = (flags & GA_RESULT_ON_DEVICE) != 0;
    hipStream_t st = ctx->work_stream();
    const size_t bytes = n * sizeof(Affine<F>);
    if (n == 1) {   // 1/n = 1 and no stage: the point itself
        const hipMemcpyKind kind = i_dev ? (o_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost) : (o_dev ? hipMemcpyHostToDevice : hipMemcpyHostToHost);
        GA_HIP_CHECK(hipMemcpyAsync(out, powers, bytes, kind, st));
        GA_HIP_CHECK(hipStreamSynchronize(st));
        return GA_OK;
    }
    const int logn = ilog2_u64(n);
    const uint64_t half = n / 2;

    // the scratch of the whole call first: an allocation failure leaves nothing in flight
    XYZZ<F>* work;
    uint32_t* tw;
    RedoList redo;   // header: the stage's count, pad
    Affine<F>* io = nullptr;
    GA_CHECK(ctx->scratch_get("ec_ntt_work", n * sizeof(XYZZ<F>), (void**)&work));
    GA_CHECK(ctx->scratch_get("ec_ntt_twiddles", half * 32, (void**)&tw));
    GA_CHECK(redo.get(ctx, "ec_ntt_redo", half, 4));
    if (!i_dev || !o_dev) GA_CHECK(ctx->scratch_get("ec_ntt_io", bytes, (void**)&io));
    uint32_t *count = redo.words, *list = redo.list;
    StreamDrain drain{st};

    Fe<FrP> winv = fe_const<FrP>(FrP::ROOT_INV);
    for (int k = 0; k < FrP::ADICITY - logn; k++) winv = sqr(winv);
    Fe<FrP> nn = fe_zero<FrP>();
    nn.l[0] = (uint32_t)n;
    nn.l[1] = (uint32_t)((uint64_t)n >> 32);
    const Fe<FrP> ninv_mont = inv(to_mont(nn));

    const Affine<F>* src;
    GA_CHECK(chunk_in(st, i_dev, (const Affine<F>*)powers, 0, n, io, &src));
    {
        StageTimer tm(ctx, "ec_ntt_setup");
        hipLaunchKernelGGL((ec_ntt_twiddle_kernel<FrP>), dim3((unsigned)((half + 255) / 256)), dim3(256), 0, st, tw, half, winv);
        hipLaunchKernelGGL((ec_ntt_load_kernel<F>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, (uint64_t)n, work);
        GA_KERNEL_CHECK();
    }
    constexpr unsigned T = Table29<F>::THREADS;
    const unsigned blocks = (unsigned)((half + T - 1) / T);
    const unsigned exact_blocks = capped_grid(half, 64, EC_NTT_EXACT_MAX_BLOCKS);
    for (int s = 0; s < logn; s++) {
        char name[32];
        snprintf(name, sizeof(name), "ec_ntt_stage_%02d", s);
        GA_HIP_CHECK(hipMemsetAsync(count, 0, 16, st));
        StageTimer tm(ctx, name);
        hipLaunchKernelGGL((ec_ntt_stage_kernel<F, FrP>), dim3(blocks), dim3(T), 0, st, work, (const uint32_t*)tw, half, s, logn, uniform, ninv_mont, list, count);
        hipLaunchKernelGGL((ec_ntt_exact_kernel<F, FrP>), dim3(exact_blocks), dim3(64), 0, st, work, (const uint32_t*)tw, s, logn, uniform, ninv_mont,
                           (const uint32_t*)list, (const uint32_t*)count);
        GA_KERNEL_CHECK();
    }
    {
        StageTimer tm(ctx, "ec_ntt_scale");
        hipLaunchKernelGGL((ec_ntt_scale_kernel<F, FrP>), dim3(1), dim3(T), 0, st, work, 1u, from_mont(ninv_mont));
        GA_KERNEL_CHECK();
    }
    GA_CHECK(launch_to_affine<F>(ctx, st, "ec_ntt_affine", work, (uint32_t)n, 0, logn, o_dev ? (Affine<F>*)out : io));
    GA_CHECK(chunk_out(st, o_dev, (Affine<F>*)out, 0, n, io));
    GA_HIP_CHECK(hipStreamSynchronize(st));
    return GA_OK;
}

// what ec_ntt_<curve>[_g2].hip instantiates
#define GA_INSTANTIATE_EC_NTT(C, G) template int ec_ntt_to_lagrange<C, G>(Ctx*, const void*, size_t, unsigned, void*, int);

}  // namespace ga

// Per-point scalar multiplication: out[i] = [s_i] points[i] for n points and n scalars -- the curve work of the Groth16 MPC ceremony
// (backend/groth16/<curve>/mpcsetup: SrsCommons.update, phase1.go:104-147, multiplies the i-th point of every SRS vector by c tau^i;
// Phase2.update, phase2.go:110-135, multiplies Z and PKK by 1/delta and SigmaCKK[i] by sigma_i).  Every base is used once, so there is
// no table to share (fixed_base.hip.h) and nothing to sum (msm.hip.h).
//
// On the context's work stream, one host synchronisation (device-resident points, scalars and output), per chunk of points:
//   1. scale_points_scalars_kernel
//        the three modes -> ONE canonical scalar (8 words, < r) per lane in scratch: GA_SCALE_EACH reduces (Montgomery or canonical
//        input), GA_SCALE_ONE broadcasts, GA_SCALE_POWERS computes c t^(first + i) with pow_u64 -- 64 Fr squarings beside ~3000 Fp
//        products, so there is no prefix scan.
//   2. scale_points_window_kernel
//        one lane per point.  The table [1..8]P (4 dbl29 + 3 add29, msm_lazy.hip.h) goes to device scratch in the packed hat format
//        (what ec_ntt_pack writes), entry-major: entry e of point i at table[e * n + i], so the lanes of a wave that share a digit
//        gather consecutive lines (an entry is 128 - 384 B: a whole number of lines of its own whatever the neighbours' digits are).
//        The scalar becomes signed 4-bit digits in [-8, 8] (64 windows and the carry-out digit); the accumulator stays in registers:
//        the top digit loads its entry, every window below it is 4 dbl29 and one add29 of the gathered entry (y negated with
//        f29_sub<2>(0, y) for a negative digit), a zero digit skips the addition.  Nothing is branched on inside the loop: an
//        exceptional addition or doubling leaves ZZ == 0 (mod p), which is absorbing, so ONE exact test of the accumulator flags the
//        lane; a lane whose table holds a point at infinity (a point of order <= 8: packed ZZ == 0) is flagged too.  Lanes with (0,0)
//        or a zero scalar write infinity and are done.
//      scale_points_plain_kernel
//        GA_SCALE_WINDOW=0: the plain double-and-add of ec_ntt.hip.h (ec_ntt_scalar_mul29, unchanged) in the same driver -- the A/B
//        baseline of tools/scale_points_bench.py.
//   3. scale_points_exact_kernel
//        the flagged lanes once more with the complete formulas of ec.hip.h (scalar_mul), grid-stride over the redo list in one-wave
//        workgroups like ec_ntt_exact_kernel (ec_ntt.hip.h: EC_NTT_EXACT_MAX_BLOCKS).
//   4. fixed_base_affine_kernel (fixed_base.hip.h)  XYZZ -> affine, dense.
// Bounds of the unreduced sequence, G1 and G2: tools/lazy_bounds.py check_ladder(curve, fp2).
#pragma once
#include "ec_ntt.hip.h"   // ec_ntt_scalar_mul29, ec_ntt_pack / _unpack / _to_exact / _from_exact, affine_to_lazy4; vec_call.hip.h
#include "fr_powers.hip.h"   // fr_canonical, fr_power_term

namespace ga {

constexpr uint64_t SCALE_DEFAULT_CHUNK = 1ull << 20;   // points per pass: 1.2 GiB (BN254 G1) .. 3.5 GiB (BLS12-381 G2) of scratch
constexpr int SCALE_TABLE = 8;                         // entries per point: [1..8]P
constexpr unsigned SCALE_MAX_BLOCKS = 1024;            // workgroups of a ladder launch (grid-stride beyond): two to four per CU
constexpr int SCALE_WINDOWS = 64;                      // 4-bit windows of a 256-bit scalar; digit 64 is the carry out of the last one

// waves per SIMD asked of the two ladder kernels: EC_NTT_MIN_WAVES as in ec_ntt_stage_kernel, except over Fp2 with 14-limb coordinates,
// where one extended point is 112 registers: under a 256-register budget the windowed kernel spilled 2130 of them (2.3 KiB of scratch
// per lane) and ran 1.25x SLOWER than the plain ladder; with the whole register file of a SIMD lane (one wave) it does not
template <class F> struct ScaleLadder {
    static constexpr int MIN_WAVES = (Lazy<F>::FP2 && BaseFieldOf<F>::P::N > 8) ? 1 : EC_NTT_MIN_WAVES;
};

// lane i of the chunk: its canonical scalar
template <class FrP>
__global__ void __launch_bounds__(256)
scale_points_scalars_kernel(const uint32_t* __restrict__ in, uint32_t n, int mode, int mont, const Fe<FrP> a, const Fe<FrP> b, uint64_t first,
                            uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fe<FrP> s;
    if (mode == GA_SCALE_EACH) s = fr_canonical(load_fe<FrP>(in + (uint64_t)i * 8), mont);
    else if (mode == GA_SCALE_ONE) s = fr_canonical(a, mont);
    else s = fr_power_term(a, b, mont, first + i);   // fr_powers.hip.h: shared with ga_fr_powers
    store_pod(out + (uint64_t)i * 8, s);
}

// Signed 4-bit digits of a canonical scalar, any window at any time: digit_w = nibble_w + carry_w - 16 carry_(w+1) with carry_(w+1) =
// [nibble_w + carry_w > 8].  carry_w is the carry INTO bit 4w of s + 0x77..7 (the low 4w bits exceed 0x88..8 exactly then), which
// is bit 4w of (s + 0x77..7) ^ s ^ 0x77..7.  The scalar and the carry word live in the lane's LDS column (dynamic word index).
struct ScaleDigits {
    uint32_t* col;
    uint32_t stride;
    __device__ __forceinline__ ScaleDigits(uint32_t* c, uint32_t st) : col(c), stride(st) {}
    __device__ __forceinline__ void set(const uint32_t (&s)[8]) {
        uint32_t carry = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint64_t t = (uint64_t)s[k] + 0x77777777u + carry;
            col[k * stride] = s[k];
            col[(8 + k) * stride] = (uint32_t)t ^ s[k] ^ 0x77777777u;
            carry = (uint32_t)(t >> 32);
        }
        col[16 * stride] = carry;
    }
    __device__ __forceinline__ uint32_t carry_in(int w) const { return (col[(8 + (w >> 3)) * stride] >> (4 * (w & 7))) & 1u; }
    __device__ __forceinline__ int digit(int w) const {   // w <= SCALE_WINDOWS
        const uint32_t nib = w < SCALE_WINDOWS ? (col[(w >> 3) * stride] >> (4 * (w & 7))) & 15u : 0u;
        const uint32_t out = w < SCALE_WINDOWS ? carry_in(w + 1) : 0u;
        return (int)(nib + carry_in(w)) - 16 * (int)out;
    }
};

// table[e * n + i] = [e + 1] P_i, packed; returns true when an entry is a point at infinity (an exceptional step on the way to it).
// One point is live at a time: what a step needs beside it comes back from the table (packed entries unpack without arithmetic).
template <class F>
__device__ __forceinline__ bool scale_build_table(const Affine<F>& P, XYZZ<F>* __restrict__ table, uint64_t n, uint64_t i) {
    bool degenerate = false;
    auto put = [&](int m, const Lazy4<F>& v) {
        const XYZZ<F> q = ec_ntt_pack<F>(v);
        degenerate |= is_zero(q.zz);
        store_pod(&table[(uint64_t)(m - 1) * n + i], q);
    };
    auto get = [&](int m) { return ec_ntt_unpack<F>(load_pod<XYZZ<F>>(&table[(uint64_t)(m - 1) * n + i])); };
    Lazy4<F> t = affine_to_lazy4<F>(P);
    put(1, t);
    dbl29<F>(t);
    put(2, t);
    add29<F>(t, get(1));
    put(3, t);
    dbl29<F>(t);
    put(6, t);
    add29<F>(t, get(1));
    put(7, t);
    t = get(2);
    dbl29<F>(t);
    put(4, t);
    dbl29<F>(t);
    put(8, t);
    t = get(4);
    add29<F>(t, get(1));
    put(5, t);
    return degenerate;
}

template <class F>
__device__ __forceinline__ void scale_store_inf(XYZZ<F>* dst) {
    const F z = FieldTraits<F>::zero();
    store_pod(dst, XYZZ<F>{z, z, z, z});
}

template <class F>
__global__ void __launch_bounds__(Table29<F>::THREADS, ScaleLadder<F>::MIN_WAVES)
scale_points_window_kernel(const Affine<F>* __restrict__ points, const uint32_t* __restrict__ scalars, uint32_t n, XYZZ<F>* __restrict__ table,
                           XYZZ<F>* __restrict__ sums, uint32_t* __restrict__ redo, uint32_t* __restrict__ redo_count) {
    constexpr unsigned T = Table29<F>::THREADS;
    __shared__ uint32_t lds[17 * T];
    ScaleDigits D(lds + threadIdx.x, T);
    // (grid-stride: the private segment is allocated per resident wave of the launch -- SCALE_MAX_BLOCKS bounds it whatever n is)
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const Affine<F> P = load_pod<Affine<F>>(&points[i]);
        uint32_t s[8], any = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) any |= s[k] = scalars[(uint64_t)i * 8 + k];
        if (is_inf(P) | (any == 0)) {
            scale_store_inf<F>(&sums[i]);
            continue;
        }
        D.set(s);
        bool flagged = scale_build_table<F>(P, table, n, i);
        int w = SCALE_WINDOWS;
        while (D.digit(w) == 0) w--;   // the top non-zero digit of a positive integer is positive
        Lazy4<F> acc = ec_ntt_unpack<F>(load_pod<XYZZ<F>>(&table[(uint64_t)(D.digit(w) - 1) * n + i]));
        for (w--; w >= 0; w--) {
#pragma unroll 1
            for (int k = 0; k < 4; k++) dbl29<F>(acc);
            const int d = D.digit(w);
            if (d != 0) {
                Lazy4<F> e = ec_ntt_unpack<F>(load_pod<XYZZ<F>>(&table[(uint64_t)((d < 0 ? -d : d) - 1) * n + i]));
                if (d < 0) e.y = f29_sub<2>(Lazy<F>::from_mem(FieldTraits<F>::zero()), e.y);   // 2p - y
                add29<F>(acc, e);
            }
        }
        flagged |= f29_is_zero_mod_p(acc.zz);
        if (flagged) redo[atomicAdd(redo_count, 1u)] = i;
        else store_pod(&sums[i], ec_ntt_pack<F>(acc));
    }
}

// the plain ladder: one doubling per bit below the top one, one addition per set bit (the base in the lane's LDS column)
template <class F>
__global__ void __launch_bounds__(Table29<F>::THREADS, ScaleLadder<F>::MIN_WAVES)
scale_points_plain_kernel(const Affine<F>* __restrict__ points, const uint32_t* __restrict__ scalars, uint32_t n, XYZZ<F>* __restrict__ sums,
                   uint32_t* __restrict__ redo, uint32_t* __restrict__ redo_count) {
    constexpr int NW = Lazy<F>::NW;
    __shared__ uint32_t lds[4 * NW * Table29<F>::THREADS];
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const Affine<F> P = load_pod<Affine<F>>(&points[i]);
        uint32_t s[8], any = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) any |= s[k] = scalars[(uint64_t)i * 8 + k];
        if (is_inf(P) | (any == 0)) {
            scale_store_inf<F>(&sums[i]);
            continue;
        }
        Lazy4<F> acc = affine_to_lazy4<F>(P);
        ec_ntt_scalar_mul29<F>(acc, LdsAcc29<F>(lds + threadIdx.x), s);
        if (f29_is_zero_mod_p(acc.zz)) redo[atomicAdd(redo_count, 1u)] = i;
        else store_pod(&sums[i], ec_ntt_pack<F>(acc));
    }
}

// the flagged lanes of a chunk with the complete formulas; lane 0 adds their number to the call's total (the kernels of a call run
// one after the other on one stream)
template <class F>
__global__ void __launch_bounds__(64)
scale_points_exact_kernel(const Affine<F>* __restrict__ points, const uint32_t* __restrict__ scalars, XYZZ<F>* __restrict__ sums,
                   const uint32_t* __restrict__ redo, const uint32_t* __restrict__ redo_count, uint64_t* __restrict__ total) {
    const uint32_t nredo = *redo_count;
    if (blockIdx.x == 0 && threadIdx.x == 0) *total += nredo;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < nredo; r += gridDim.x * blockDim.x) {
        const uint32_t i = redo[r];
        uint32_t s[8];
#pragma unroll
        for (int k = 0; k < 8; k++) s[k] = scalars[(uint64_t)i * 8 + k];
        store_pod(&sums[i], ec_ntt_from_exact<F>(scalar_mul(to_xyzz(load_pod<Affine<F>>(&points[i])), s, 8)));
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// windowed: 1 = the signed 4-bit windows (default), 0 = the plain ladder (GA_SCALE_WINDOW); forced_chunk: GA_SCALE_CHUNK (0 = default)
template <class C, int G>
int scale_points_run(Ctx* ctx, const void* points, size_t n, int mode, const void* scalars, uint64_t first, unsigned flags, void* out,
                     uint64_t* redone, int windowed, uint64_t forced_chunk) {
    typedef typename GroupField<C, G>::F F;
    typedef typename C::FrP FrP;
    const bool mont = (flags & GA_SCALARS_MONTGOMERY) != 0, s_dev = (flags & GA_SCALARS_ON_DEVICE) != 0;
    const bool i_dev = (flags & GA_BASES_ON_DEVICE) != 0, o_dev = (flags & GA_RESULT_ON_DEVICE) != 0;
    const uint64_t chunk = clamp_chunk(forced_chunk, SCALE_DEFAULT_CHUNK, n);
    hipStream_t st = ctx->work_stream();

    // the scratch of the whole call first: an allocation failure leaves nothing in flight
    XYZZ<F>*table = nullptr, *sums;
    uint32_t *canon, *d_scalars = nullptr;
    RedoList redo;   // header: the call's total (64 bits), the chunk's count, pad
    Affine<F>* io = nullptr;
    if (windowed) GA_CHECK(ctx->scratch_get("scale_table", SCALE_TABLE * chunk * sizeof(XYZZ<F>), (void**)&table));
    GA_CHECK(ctx->scratch_get("scale_sums", chunk * sizeof(XYZZ<F>), (void**)&sums));
    GA_CHECK(ctx->scratch_get("scale_canonical", chunk * 32, (void**)&canon));
    GA_CHECK(redo.get(ctx, "scale_redo", chunk, 8));
    if (mode == GA_SCALE_EACH && !s_dev) GA_CHECK(ctx->scratch_get("scale_scalars", chunk * 32, (void**)&d_scalars));
    if (!i_dev || !o_dev) GA_CHECK(ctx->scratch_get("scale_io", chunk * sizeof(Affine<F>), (void**)&io));
    uint64_t* total = (uint64_t*)redo.words;
    uint32_t *count = redo.words + 2, *list = redo.list;
    StreamDrain drain{st};

    Fe<FrP> a = fe_zero<FrP>(), b = fe_zero<FrP>();
    if (mode != GA_SCALE_EACH) memcpy(&a, scalars, 32);
    if (mode == GA_SCALE_POWERS) memcpy(&b, (const char*)scalars + 32, 32);
    uint64_t h_total = 0;
    GA_HIP_CHECK(hipMemsetAsync(total, 0, 8, st));

    constexpr unsigned T = Table29<F>::THREADS;
    for (uint64_t done = 0; done < n; done += chunk) {
        const uint32_t cn = (uint32_t)(n - done < chunk ? n - done : chunk);
        const uint32_t* sc = nullptr;
        if (mode == GA_SCALE_EACH) GA_CHECK(chunk_in(st, s_dev, (const uint32_t*)scalars, done * 8, (uint64_t)cn * 8, d_scalars, &sc));
        // the chunk's points: read where they are on the device, else staged; the staging buffer also takes a host-bound result (the
        // affine kernel is the last reader of nothing but the sums, so input and output may share it -- as they do for out == points)
        const Affine<F>* src;
        GA_CHECK(chunk_in(st, i_dev, (const Affine<F>*)points, done, cn, io, &src));
        GA_HIP_CHECK(hipMemsetAsync(count, 0, 8, st));
        {
            StageTimer tm(ctx, "scale_scalars");
            hipLaunchKernelGGL((scale_points_scalars_kernel<FrP>), dim3((cn + 255) / 256), dim3(256), 0, st, sc, cn, mode, (int)mont, a, b, first + done, canon);
            GA_KERNEL_CHECK();
        }
        {
            StageTimer tm(ctx, "scale_ladder");
            const unsigned blocks = capped_grid(cn, T, SCALE_MAX_BLOCKS), exact_blocks = capped_grid(cn, 64, EC_NTT_EXACT_MAX_BLOCKS);
            if (windowed)
                hipLaunchKernelGGL((scale_points_window_kernel<F>), dim3(blocks), dim3(T), 0, st, src, (const uint32_t*)canon, cn, table, sums, list, count);
            else
                hipLaunchKernelGGL((scale_points_plain_kernel<F>), dim3(blocks), dim3(T), 0, st, src, (const uint32_t*)canon, cn, sums, list, count);
            hipLaunchKernelGGL((scale_points_exact_kernel<F>), dim3(exact_blocks), dim3(64), 0, st, src, (const uint32_t*)canon, sums, (const uint32_t*)list,
                               (const uint32_t*)count, total);
            GA_KERNEL_CHECK();
        }
        GA_CHECK(launch_to_affine<F>(ctx, st, "scale_affine", sums, cn, o_dev ? done : 0, -1, o_dev ? (Affine<F>*)out : io));
        GA_CHECK(chunk_out(st, o_dev, (Affine<F>*)out, done, cn, io));
    }
    GA_HIP_CHECK(hipMemcpyAsync(&h_total, total, 8, hipMemcpyDeviceToHost, st));
    GA_HIP_CHECK(hipStreamSynchronize(st));   // the one synchronisation of a call with everything on the device
    if (redone) *redone = h_total;
    return GA_OK;
}

// what scale_points_<curve>_g<k>.hip instantiates
#define GA_INSTANTIATE_SCALE_POINTS(C, G) \
    template int scale_points_run<C, G>(Ctx*, const void*, size_t, int, const void*, uint64_t, unsigned, void*, uint64_t*, int, uint64_t);

}  // namespace ga

// Fixed-base batch scalar multiplication: out[i] = [s_i] B for ONE base B and n full-width scalars, n affine points out.
//
// Replaces curve.BatchScalarMultiplicationG1 / G2 as groth16.Setup calls them (backend/groth16/bn254/setup.go:233,302: all the curve
// work of a trusted setup, ~3 nbWires + n scalars in G1, ~nbWires in G2) and as kzg.NewSRS does over the powers of tau.
//
// Three stages on the context's work stream, one host synchronisation (device-resident scalars and output):
//   1. fixed_base_table_kernel       T[w][j] = [(j+1) 2^(c w)] B for j < 2^(c-1) and every window w (signed c-bit digits, the
//                                    recoding of the MSM: DigitWalk, msm_sort.hip.h), in the packed hat format the bucket kernel
//                                    gathers (Table29<F>::WORDS per entry, (0,0) = infinity).  The window bases [2^(c w)] B -- one
//                                    chain of BITS sequential doublings -- come from the host (a chain of dependent doublings is
//                                    latency-bound on a GPU lane and free on a host core, as in the MSM's tail); the 2^(c-1)
//                                    multiples of each are built on the device: a lane double-and-adds to its first entry, walks K
//                                    consecutive entries by adding the window base, and converts them to affine with ONE inversion.
//   2. fixed_base_accumulate_kernel  one lane per scalar: Montgomery reduction, signed digits, `windows` lazy mixed additions
//                                    (madd29) of gathered table entries into an XYZZ accumulator in LDS.  Exceptional additions are
//                                    not branched on: ONE exact ZZ == 0 test per scalar flags the lane; flagged scalars go through a
//                                    redo list to the complete lazy loop (madd29_complete) and what that cannot finish to the exact
//                                    arithmetic.  A degenerate base (small order: every lane flagged) is slow and right.
//   3. fixed_base_affine_kernel      XYZZ -> affine with Montgomery's trick inside the lane (K points, one f29_inv), written dense or
//                                    at the bit-reversed index (setup.go:247), gnark's Montgomery image, (0,0) for infinity.
// The scalars are walked in chunks (GA_FIXED_BASE_CHUNK), so the scratch is bounded for any n and host input / output stream
// through it.
#pragma once
#include "keyio.hip.h"        // CurveB: the on-curve test of the base
#include "msm_bucket.hip.h"   // Table29, LdsAcc29, load_point29, madd29 / madd29_complete; DigitWalk (msm_sort.hip.h)
#include "vec_call.hip.h"     // the driver kit: StreamDrain, clamp_chunk, capped_grid, RedoList, chunk_in / chunk_out

namespace ga {

constexpr int FB_MAX_C = 18;                         // widest PLANNED window: 15 x 2^17 entries (120 MiB for BN254 G1)
constexpr int FB_MAX_FORCED_C = 20;                  // widest window GA_FIXED_BASE_C may force (13 x 2^19 entries); narrowest: 2
constexpr unsigned FB_TABLE_MAX_BLOCKS = 2048;       // one-wave workgroups of the table build (two per SIMD: the kernel's occupancy)
constexpr uint64_t FB_DEFAULT_CHUNK = 1ull << 22;    // scalars per pass: 0.9 GiB (BN254 G1) .. 2.4 GiB (BLS12-381 G2) of scratch

// points per lane that share one inversion: the table build (exact arithmetic, K consecutive multiples) and stage 3 (lazy)
template <class F> struct FixedBaseBatch {
    static constexpr int TABLE_K = BaseFieldOf<F>::IS_FP ? 8 : 4;   // (K points + K prefix products live in the lane's private segment: <= 2 KiB)
    static constexpr int AFFINE_K = BaseFieldOf<F>::IS_FP ? (BaseFieldOf<F>::P::N <= 8 ? 8 : 4) : (BaseFieldOf<F>::P::N <= 8 ? 4 : 2);
};

// Window width: table build + n * windows additions, in mixed-addition equivalents.  A table entry costs ~3c/K + 10 of them (its
// share of the lane's double-and-add, one addition, its share of the inversion).  Deterministic in (curve, n); planned widths are 4 .. FB_MAX_C,
// GA_FIXED_BASE_C forces 2 .. FB_MAX_FORCED_C.
template <class C>
inline void fixed_base_plan(size_t n, int forced_c, int* c_out, int* nwin_out) {
    const int bits = C::FrP::BITS;
    int bc = forced_c;
    if (bc < 2 || bc > FB_MAX_FORCED_C) {   // (no or an unusable GA_FIXED_BASE_C: plan)
        double best = 1e300;
        bc = 4;
        for (int c = 4; c <= FB_MAX_C; c++) {
            const int nwin = bits / c + 1;
            const double cost = (double)nwin * ((double)(1u << (c - 1)) * (3.0 * c / 8 + 10.0) + (double)n);
            if (cost < best) {
                best = cost;
                bc = c;
            }
        }
    }
    *c_out = bc;
    *nwin_out = bits / bc + 1;
}

GA_HD uint64_t fixed_base_bitrev(uint64_t v, int bits) {
    uint64_t r = 0;
    for (int k = 0; k < bits; k++) {
        r = (r << 1) | (v & 1);
        v >>= 1;
    }
    return r;
}

// ---- 1. the window table ---------------------------------------------------------------------------------------------------------
// A lane owns kk = min(K, 2^(c-1)) consecutive entries of one window: [m0] W by double-and-add (complete exact formulas: W may be
// any curve point, of small order or at infinity), then m0 + 1, ... by adding W; batch to affine; hat domain.
template <class F>
__global__ void __launch_bounds__(64)
fixed_base_table_kernel(const Affine<F>* __restrict__ win_bases, int c, int nwin, uint32_t* __restrict__ table) {
    constexpr int K = FixedBaseBatch<F>::TABLE_K;
    const uint32_t half = 1u << (c - 1);
    const uint32_t kk = half < (uint32_t)K ? half : (uint32_t)K;
    const uint64_t entries = (uint64_t)nwin * half;
    // (grid-stride: the exact point arithmetic keeps 1.5 - 4.6 KiB per lane in the private segment, which the runtime allocates per
    // resident wave of the launch -- FB_TABLE_MAX_BLOCKS waves bound it whatever the table's size)
    for (uint64_t first = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * kk; first < entries; first += (uint64_t)gridDim.x * blockDim.x * kk) {
        const Affine<F> W = load_pod<Affine<F>>(&win_bases[first >> (c - 1)]);
        const uint32_t m0 = (uint32_t)(first & (half - 1)) + 1;
        XYZZ<F> pts[K];
        XYZZ<F> r = xyzz_inf<F>();
        for (int b = c - 1; b >= 0; b--) {
            r = dbl(r);
            if ((m0 >> b) & 1) r = madd(r, W);
        }
        pts[0] = r;
        for (uint32_t q = 1; q < kk; q++) {
            r = madd(r, W);
            pts[q] = r;
        }
        // t_q = zz_q * zzz_q (1 for a point at infinity, which stays (0,0)); one inversion of their product
        const F one = FieldTraits<F>::one();
        F pre[K];
        for (uint32_t q = 0; q < kk; q++) {
            const F t = is_inf(pts[q]) ? one : mul(pts[q].zz, pts[q].zzz);
            pre[q] = q == 0 ? t : mul(pre[q - 1], t);
        }
        F run = inv(pre[kk - 1]);
        for (uint32_t q = kk; q-- > 0;) {
            const bool at_inf = is_inf(pts[q]);
            const F it = q > 0 ? mul(run, pre[q - 1]) : run;   // 1 / t_q
            if (q > 0 && !at_inf) run = mul(run, mul(pts[q].zz, pts[q].zzz));
            Affine<F> h{FieldTraits<F>::zero(), FieldTraits<F>::zero()};
            if (!at_inf) {
                h.x = Lazy<F>::hat_packed(mul(pts[q].x, mul(it, pts[q].zzz)));   // X / zz
                h.y = Lazy<F>::hat_packed(mul(pts[q].y, mul(it, pts[q].zz)));    // Y / zzz
            }
            store_pod(table + (first + q) * Table29<F>::WORDS, h);
        }
    }
}

// ---- 2. accumulation -------------------------------------------------------------------------------------------------------------
// The sums leave stage 2 as XYZZ points whose coordinates are canonical packed hat-domain words (what f29_pack_hat writes and
// Lazy<F>::unpack reads back without arithmetic); all-zero ZZ = the point at infinity.
template <class F, class FrP, bool COMPLETE>
__device__ __forceinline__ bool fixed_base_accumulate(const LdsAcc29<F>& A, const uint32_t* __restrict__ table, const uint32_t* __restrict__ scalars,
                                                      uint64_t i, int mont, int c, int nwin) {
    typedef typename Lazy<F>::T T;
    typedef typename Lazy<F>::Params P;
    const T one = Lazy<F>::from_mem(FieldTraits<F>::one());
    const uint32_t half = 1u << (c - 1);
    DigitWalk<FrP> D;
    D.load(scalars, i, mont);
    bool have = false;
    for (int w = 0; w < nwin; w++) {
        uint32_t key, val;
        D.next(c, w, 0, 0, 0, 1, 0u, 0xFFFFFFFFu, key, val);   // key = |digit| - 1 (or the skip key), val = the sign
        if (key == 0xFFFFFFFFu) continue;
        T qx, qy;
        load_point29<F>(table, (uint32_t)w * half + key, qx, qy);
        if (f29_is_zero_limbs(qx) & f29_is_zero_limbs(qy)) continue;   // (0,0) = infinity: a base of small order
        if (val & MSM_SIGN) qy = f29_sub<2>(Lazy<F>::from_mem(FieldTraits<F>::zero()), qy);   // 2p - y
        if (!have) {
            A.put(0, qx);
            A.put(1, qy);
            A.put(2, one);
            A.put(3, one);
            have = true;
        } else if constexpr (COMPLETE) {
            have = madd29_complete<F>(A, qx, qy);
        } else {
            madd29<P>(A, qx, qy);
        }
    }
    return have;
}

// the lane's sum out of the LDS accumulator: false when an exceptional addition slipped through (ZZ == 0 mod p)
template <class F>
__device__ __forceinline__ bool fixed_base_store(const LdsAcc29<F>& A, bool have, XYZZ<F>* __restrict__ dst) {
    const F z = FieldTraits<F>::zero();
    XYZZ<F> o{z, z, z, z};
    if (have) {
        const typename Lazy<F>::T zz = A.get(2);
        if (f29_is_zero_mod_p(zz)) return false;
        o.x = f29_pack_hat(A.get(0));
        o.y = f29_pack_hat(A.get(1));
        o.zz = f29_pack_hat(zz);
        o.zzz = f29_pack_hat(A.get(3));
    }
    store_pod(dst, o);
    return true;
}

// COMPLETE = false: every scalar of the chunk, the fast loop, flagged lanes appended to redo_out.  COMPLETE = true: the scalars of
// redo_in (grid-stride) with the exceptional cases handled in place; what still ends in ZZ == 0 goes on to redo_out.
template <class F, class FrP, bool COMPLETE>
__global__ void __launch_bounds__(Table29<F>::THREADS, Table29<F>::MIN_WAVES)
fixed_base_accumulate_kernel(const uint32_t* __restrict__ table, const uint32_t* __restrict__ scalars, uint32_t n, int mont, int c, int nwin,
                             XYZZ<F>* __restrict__ sums, const uint32_t* __restrict__ redo_in, const uint32_t* __restrict__ redo_in_count,
                             uint32_t* __restrict__ redo_out, uint32_t* __restrict__ redo_out_count) {
    constexpr int NW = Lazy<F>::NW;
    __shared__ uint32_t lds[4 * NW * Table29<F>::THREADS];
    LdsAcc29<F> A(lds + threadIdx.x);
    if constexpr (!COMPLETE) {
        const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= n) return;
        const bool have = fixed_base_accumulate<F, FrP, false>(A, table, scalars, i, mont, c, nwin);
        if (!fixed_base_store<F>(A, have, &sums[i])) redo_out[atomicAdd(redo_out_count, 1u)] = i;
    } else {
        const uint32_t nredo = *redo_in_count;
        for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < nredo; r += gridDim.x * blockDim.x) {
            const uint32_t i = redo_in[r];
            const bool have = fixed_base_accumulate<F, FrP, true>(A, table, scalars, i, mont, c, nwin);
            if (!fixed_base_store<F>(A, have, &sums[i])) redo_out[atomicAdd(redo_out_count, 1u)] = i;
        }
    }
}

// exact re-run of the scalars on a redo list (complete formulas; table points converted back to gnark's form)
template <class F, class FrP>
__global__ void __launch_bounds__(64)
fixed_base_exact_kernel(const uint32_t* __restrict__ table, const uint32_t* __restrict__ scalars, int mont, int c, int nwin,
                        XYZZ<F>* __restrict__ sums, const uint32_t* __restrict__ redo, const uint32_t* __restrict__ redo_count) {
    typedef typename Lazy<F>::T T;
    const uint32_t half = 1u << (c - 1);
    const uint32_t nredo = *redo_count;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < nredo; r += gridDim.x * blockDim.x) {
        const uint32_t i = redo[r];
        DigitWalk<FrP> D;
        D.load(scalars, i, mont);
        XYZZ<F> acc = xyzz_inf<F>();
        for (int w = 0; w < nwin; w++) {
            uint32_t key, val;
            D.next(c, w, 0, 0, 0, 1, 0u, 0xFFFFFFFFu, key, val);
            if (key == 0xFFFFFFFFu) continue;
            T qx, qy;
            load_point29<F>(table, (uint32_t)w * half + key, qx, qy);
            Affine<F> q{Lazy<F>::to_mem(qx), Lazy<F>::to_mem(qy)};
            if (val & MSM_SIGN) q.y = neg(q.y);
            acc = madd(acc, q);
        }
        const F z = FieldTraits<F>::zero();
        XYZZ<F> o{z, z, z, z};
        if (!is_inf(acc)) o = {Lazy<F>::hat_packed(acc.x), Lazy<F>::hat_packed(acc.y), Lazy<F>::hat_packed(acc.zz), Lazy<F>::hat_packed(acc.zzz)};
        store_pod(&sums[i], o);
    }
}

// ---- 3. to affine ----------------------------------------------------------------------------------------------------------------
// Point q of a lane is gid + q * lanes (coalesced).  Pass 1 reads ZZ, ZZZ and keeps the prefix products of t_q = zz_q * zzz_q (points
// at infinity stay out of the product); one inversion; pass 2 reads the points again, last first.  Output index: first + i, or its
// bit reversal over logn bits (logn >= 0).
template <class F>
__global__ void __launch_bounds__(64)
fixed_base_affine_kernel(const XYZZ<F>* __restrict__ sums, uint32_t n, uint64_t first, int logn, Affine<F>* __restrict__ out) {
    typedef typename Lazy<F>::T T;
    constexpr int K = FixedBaseBatch<F>::AFFINE_K;
    const uint32_t lanes = gridDim.x * blockDim.x;
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n) return;
    const T one = Lazy<F>::from_mem(FieldTraits<F>::one());
    T pre[K];
    bool inf[K];
#pragma unroll
    for (int q = 0; q < K; q++) {
        const uint64_t i = (uint64_t)gid + (uint64_t)q * lanes;
        T t = one;
        inf[q] = true;
        if (i < n) {
            const F zz = load_pod<F>(&sums[i].zz);
            if (!is_zero(zz)) {
                inf[q] = false;
                t = f29_mul(Lazy<F>::unpack(zz), Lazy<F>::unpack(load_pod<F>(&sums[i].zzz)));
            }
        }
        pre[q] = q == 0 ? t : f29_mul(pre[q - 1], t);
    }
    T run = f29_inv(pre[K - 1]);
#pragma unroll
    for (int q = K - 1; q >= 0; q--) {
        const uint64_t i = (uint64_t)gid + (uint64_t)q * lanes;
        if (i >= n) continue;   // (t_q = 1: run needs no update)
        Affine<F> a{FieldTraits<F>::zero(), FieldTraits<F>::zero()};
        if (!inf[q]) {
            const XYZZ<F> p = load_pod<XYZZ<F>>(&sums[i]);
            const T zz = Lazy<F>::unpack(p.zz), zzz = Lazy<F>::unpack(p.zzz);
            const T it = q > 0 ? f29_mul(run, pre[q - 1]) : run;   // 1 / t_q
            if (q > 0) run = f29_mul(run, f29_mul(zz, zzz));
            a.x = Lazy<F>::to_mem(f29_mul(Lazy<F>::unpack(p.x), f29_mul(it, zzz)));   // X / zz
            a.y = Lazy<F>::to_mem(f29_mul(Lazy<F>::unpack(p.y), f29_mul(it, zz)));    // Y / zzz
        }
        const uint64_t g = first + i;
        store_pod(&out[logn >= 0 ? fixed_base_bitrev(g, logn) : g], a);
    }
}

// stage 3 as the point drivers launch it: out[first + i], or its bit reversal over logn >= 0 bits, i < n
template <class F>
int launch_to_affine(Ctx* ctx, hipStream_t st, const char* stage_name, const XYZZ<F>* sums, uint32_t n, uint64_t first, int logn, Affine<F>* out) {
    StageTimer tm(ctx, stage_name, st);
    constexpr unsigned K = (unsigned)FixedBaseBatch<F>::AFFINE_K;
    hipLaunchKernelGGL((fixed_base_affine_kernel<F>), dim3(((n + K - 1) / K + 63) / 64), dim3(64), 0, st, sums, n, first, logn, out);
    GA_KERNEL_CHECK();
    return GA_OK;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
template <class C, int G>
int fixed_base_run(Ctx* ctx, const void* h_base, const void* scalars, size_t n, unsigned flags, void* out, int forced_c, uint64_t forced_chunk) {
    typedef typename GroupField<C, G>::F F;
    typedef typename C::FrP FrP;
    Affine<F> base;
    memcpy(&base, h_base, sizeof(base));
    if (!is_inf(base) && !eq(sqr(base.y), add(mul(sqr(base.x), base.x), CurveB<F>::get()))) {
        set_error("ga_batch_scalar_mul: the base is not a point of the curve");
        return GA_ERR_INVALID;
    }
    const bool mont = (flags & GA_SCALARS_MONTGOMERY) != 0, s_dev = (flags & GA_SCALARS_ON_DEVICE) != 0;
    const bool o_dev = (flags & GA_RESULT_ON_DEVICE) != 0, bitrev = (flags & GA_RESULT_BITREVERSED) != 0;
    const int logn = bitrev ? ilog2_u64(n) : -1;
    int c, nwin;
    fixed_base_plan<C>(n, forced_c, &c, &nwin);
    const uint32_t half = 1u << (c - 1);
    const uint64_t entries = (uint64_t)nwin * half;
    const uint64_t chunk = clamp_chunk(forced_chunk, FB_DEFAULT_CHUNK, n);
    hipStream_t st = ctx->work_stream();

    // the scratch of the whole call first: an allocation failure leaves nothing in flight
    Affine<F>* d_win;
    uint32_t *table, *d_scalars = nullptr;
    RedoList redo;   // header: the counts of the two lists; list 1 (the fast loop's) | list 2 (the complete lazy loop's), chunk words each
    XYZZ<F>* sums;
    Affine<F>* d_out = nullptr;
    GA_CHECK(ctx->scratch_get("fb_win_bases", (size_t)nwin * sizeof(Affine<F>), (void**)&d_win));
    GA_CHECK(ctx->scratch_get("fb_table", entries * Table29<F>::WORDS * 4 + 256, (void**)&table));
    GA_CHECK(ctx->scratch_get("fb_sums", chunk * sizeof(XYZZ<F>), (void**)&sums));
    GA_CHECK(redo.get(ctx, "fb_redo", 2 * chunk, 4));
    if (!s_dev) GA_CHECK(ctx->scratch_get("fb_scalars", chunk * 32, (void**)&d_scalars));
    if (!o_dev) GA_CHECK(ctx->scratch_get("fb_out", chunk * sizeof(Affine<F>), (void**)&d_out));
    uint32_t *count = redo.words, *list1 = redo.list, *list2 = redo.list + chunk;
    std::vector<Affine<F>> h_stage(!o_dev && bitrev ? chunk : 0);   // host output at bit-reversed indices: permuted here
    std::vector<Affine<F>> win((size_t)nwin);
    StreamDrain drain{st};

    // 1. window bases on the host (BITS sequential doublings), their multiples on the device
    {
        XYZZ<F> p = to_xyzz(base);
        for (int w = 0; w < nwin; w++) {
            win[w] = to_affine(p);
            if (w + 1 < nwin)
                for (int k = 0; k < c; k++) p = dbl(p);
        }
    }
    GA_HIP_CHECK(hipMemcpyAsync(d_win, win.data(), win.size() * sizeof(Affine<F>), hipMemcpyHostToDevice, st));
    {
        StageTimer tm(ctx, "fixed_base_table");
        const uint32_t kk = half < (uint32_t)FixedBaseBatch<F>::TABLE_K ? half : (uint32_t)FixedBaseBatch<F>::TABLE_K;
        hipLaunchKernelGGL((fixed_base_table_kernel<F>), dim3(capped_grid(entries / kk, 64, FB_TABLE_MAX_BLOCKS)), dim3(64), 0, st, (const Affine<F>*)d_win, c, nwin, table);
        GA_KERNEL_CHECK();
    }

    constexpr unsigned AT = Table29<F>::THREADS;
    for (uint64_t done = 0; done < n; done += chunk) {
        const uint32_t cn = (uint32_t)(n - done < chunk ? n - done : chunk);
        const uint32_t* sc;
        GA_CHECK(chunk_in(st, s_dev, (const uint32_t*)scalars, done * 8, (uint64_t)cn * 8, d_scalars, &sc));
        GA_HIP_CHECK(hipMemsetAsync(count, 0, 16, st));
        {
            // 2. the fast loop; the lanes it flagged once more with the complete lazy loop (GA_MSM_EXACT_REDO=1, tests: straight to the
            // exact kernel); whatever is left with the exact kernel
            StageTimer tm(ctx, "fixed_base_accumulate");
            const unsigned blocks = (cn + AT - 1) / AT, redo_blocks = capped_grid(cn, AT, 1024);
            hipLaunchKernelGGL((fixed_base_accumulate_kernel<F, FrP, false>), dim3(blocks), dim3(AT), 0, st, (const uint32_t*)table, sc, cn, (int)mont, c,
                               nwin, sums, (const uint32_t*)nullptr, (const uint32_t*)nullptr, list1, count);
            if (!ctx->tun.msm_exact_redo)
                hipLaunchKernelGGL((fixed_base_accumulate_kernel<F, FrP, true>), dim3(redo_blocks), dim3(AT), 0, st, (const uint32_t*)table, sc, cn, (int)mont,
                                   c, nwin, sums, (const uint32_t*)list1, (const uint32_t*)count, list2, count + 1);
            else
                hipLaunchKernelGGL((fixed_base_exact_kernel<F, FrP>), dim3(redo_blocks), dim3(64), 0, st, (const uint32_t*)table, sc, (int)mont, c, nwin, sums,
                                   (const uint32_t*)list1, (const uint32_t*)count);
            hipLaunchKernelGGL((fixed_base_exact_kernel<F, FrP>), dim3(redo_blocks), dim3(64), 0, st, (const uint32_t*)table, sc, (int)mont, c, nwin, sums,
                               (const uint32_t*)list2, (const uint32_t*)(count + 1));
            GA_KERNEL_CHECK();
        }
        // 3. to affine: straight to its place in a device-resident output, else dense into the chunk's staging buffer
        GA_CHECK(launch_to_affine<F>(ctx, st, "fixed_base_affine", sums, cn, o_dev ? done : 0, o_dev ? logn : -1, o_dev ? (Affine<F>*)out : d_out));
        if (!o_dev) {
            Affine<F>* h_out = (Affine<F>*)out;
            if (!bitrev) {
                GA_CHECK(chunk_out(st, false, h_out, done, cn, d_out));
            } else {
                GA_HIP_CHECK(hipMemcpyAsync(h_stage.data(), d_out, (size_t)cn * sizeof(Affine<F>), hipMemcpyDeviceToHost, st));
                GA_HIP_CHECK(hipStreamSynchronize(st));
                for (uint32_t i = 0; i < cn; i++) h_out[fixed_base_bitrev(done + i, logn)] = h_stage[i];
            }
        }
    }
    GA_HIP_CHECK(hipStreamSynchronize(st));   // the one synchronisation of a call with device-resident scalars and output
    return GA_OK;
}

// the width and window count fixed_base_run will use for n scalars (ga_batch_scalar_mul_plan)
template <class C>
int fixed_base_plan_abi(size_t n, int forced_c, int* c, int* nwin) {
    fixed_base_plan<C>(n, forced_c, c, nwin);
    return GA_OK;
}

// what fixed_base_<curve>_g<k>.hip instantiates; the G1 unit of a curve has the planner as well
#define GA_INSTANTIATE_FIXED_BASE(C, G) \
    template int fixed_base_run<C, G>(Ctx*, const void*, const void*, size_t, unsigned, void*, int, uint64_t);
#define GA_INSTANTIATE_FIXED_BASE_PLAN(C) template int fixed_base_plan_abi<C>(size_t, int, int*, int*);

}  // namespace ga

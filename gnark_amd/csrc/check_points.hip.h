// Batch on-curve and prime-order-subgroup checks: what gnark-crypto's default decoder does for every point it reads
// (G1Affine / G2Affine.IsOnCurve and IsInSubGroup), for n points at once.  status[i] = GA_POINT_OK, GA_POINT_OFF_CURVE or
// GA_POINT_NOT_IN_SUBGROUP; the truth is "on the curve and [r]P = O", decided per group by an identity in the curve's 64-bit seed x0
// (constants: tools/gen_constants.py endo_constants, which asserts each identity on the generator):
//   BN254 G1      cofactor 1: the curve equation alone.
//   BLS12-381 G1, BLS12-377 G1
//                 P + [x0^2] phi(P) = O,  phi(x, y) = (BETA x, y): two ladders by |x0|, then BETA X2 = x ZZ2, Y2 = -y ZZZ2.
//   BLS12-381 G2  psi(P) = [x0] P,  x0 = -|x0|: one ladder, then psi(P) = -[|x0|]P.
//   BN254 G2      [x0 + 1]P + psi([x0]P) + psi^2([x0]P) = psi^3([2 x0]P): one ladder, five complete additions, one comparison.
//
// On the context's work stream, one host synchronisation (device-resident points and status), per chunk of points:
//   1. check_points_kernel        one lane per point.  A coordinate image not below p is GA_POINT_OFF_CURVE before any arithmetic sees
//                                 it; then y^2 = x^3 + b in the exact arithmetic (field.hip.h).  The ladder is left-to-right
//                                 double-and-add on dbl29 / add29 (msm_lazy.hip.h) over the compile-time seed: every lane of every wave
//                                 takes the same sequence, the base sits in the lane's LDS column, the accumulator in registers.
//                                 Nothing is branched on inside it: an exceptional step leaves ZZ == 0 (mod p), which is absorbing,
//                                 so ONE test at the end sends the lane to the redo list.  The result goes to the exact arithmetic
//                                 (ec_ntt_to_exact) and the endomorphism, the closing additions and the projective comparison run on
//                                 reduced values: a dozen products beside the ladder's 640 - 1300.
//      check_points_naive_kernel  GA_CHECK_NAIVE=1: the definition on the plain lazy ladder (ec_ntt_scalar_mul29), [r - 1]P = -P --
//                                 not [r]P, whose last step P + (-P) is exceptional for every honest point.  The A/B baseline of
//                                 tools/check_points_bench.py and the second opinion of the tests.
//   2. check_points_exact_kernel  the flagged lanes with the complete formulas of ec.hip.h: scalar_mul by r, infinity or not.  A point
//                                 of order r is never flagged (no partial multiple below 2^64, nor below r - 1, is 0 or +-1 mod r).
// Bounds of the unreduced sequence: tools/lazy_bounds.py check_ladder(curve, fp2) -- the base of the second BLS12-381 G1 ladder is
// an output of the first, which that fixed point covers.
#pragma once
#include "ec_ntt.hip.h"   // ec_ntt_scalar_mul29, ec_ntt_pack, ec_ntt_to_exact, affine_to_lazy4; Table29, LdsAcc29; add29, dbl29; CurveB (keyio.hip.h)

namespace ga {

constexpr uint64_t CHECK_DEFAULT_CHUNK = 1ull << 20;   // points per pass: one status byte and one redo word each
constexpr unsigned CHECK_MAX_BLOCKS = 1024;            // workgroups of a ladder launch (grid-stride beyond), as SCALE_MAX_BLOCKS (scale_points.hip.h)

enum { CHECK_RULE_CURVE = 0, CHECK_RULE_BLS_G1 = 1, CHECK_RULE_BLS_G2 = 2, CHECK_RULE_BN_G2 = 3 };

// per coordinate field: the identity and |x0|
template <class F> struct CheckRule;
template <> struct CheckRule<Fe<BN254_Fp>> {
    static constexpr int RULE = CHECK_RULE_CURVE;
    static constexpr uint64_t SEED = 0;
};
template <> struct CheckRule<Fe2<BN254_Fp>> {
    static constexpr int RULE = CHECK_RULE_BN_G2;
    static constexpr uint64_t SEED = 4965661367192848881ull;   // 63 bits, weight 28
};
template <> struct CheckRule<Fe<BLS12_381_Fp>> {
    static constexpr int RULE = CHECK_RULE_BLS_G1;
    static constexpr uint64_t SEED = 0xd201000000010000ull;    // |x0|: 64 bits, weight 6
};
template <> struct CheckRule<Fe2<BLS12_381_Fp>> {
    static constexpr int RULE = CHECK_RULE_BLS_G2;
    static constexpr uint64_t SEED = 0xd201000000010000ull;
};
template <> struct CheckRule<Fe<BLS12_377_Fp>> {               // (G1 only: no rule over Fe2 of this field, common.hip.h HAS_G2)
    static constexpr int RULE = CHECK_RULE_BLS_G1;
    static constexpr uint64_t SEED = 0x8508c00000000001ull;    // x0 > 0: 64 bits, weight 7
};

// waves per SIMD asked of the two ladder kernels (DESIGN.md 4.12 has the register figures).  The fast kernel over Fp2 takes the whole
// register file of a SIMD lane: under the two-wave bound the BN254 G2 kernel spilled 147 registers (2 with one wave) and ran 10 %
// slower at 2^18 points; BLS12-381 G2 runs 128-lane workgroups, for which both bounds mean one wave.  The naive kernel keeps the
// bounds of the plain ladder of scale_points.hip.h, which it is
template <class F> struct CheckLadder {
    static constexpr int MIN_WAVES = Lazy<F>::FP2 ? 1 : EC_NTT_MIN_WAVES;
    static constexpr int NAIVE_MIN_WAVES = (Lazy<F>::FP2 && BaseFieldOf<F>::P::N > 8) ? 1 : EC_NTT_MIN_WAVES;
};

// the per-call counters in device scratch: points off the curve, outside the subgroup, sent to the exact kernel, and per failure the
// complement of the lowest index that shows it (0 = none yet: atomicMax finds the first)
struct CheckCounters {
    unsigned long long off, outside, redone;
    uint32_t first_off_inv, first_outside_inv;
};

template <class P> GA_HD bool check_reduced(const Fe<P>& a) { return !geq_mod<P>(a.l); }
template <class P> GA_HD bool check_reduced(const Fe2<P>& a) { return !geq_mod<P>(a.c0.l) & !geq_mod<P>(a.c1.l); }

// images below p and y^2 = x^3 + b; (0,0) is the caller's case
template <class F>
__device__ __forceinline__ bool check_on_curve(const Affine<F>& p) {
    if (!(check_reduced(p.x) & check_reduced(p.y))) return false;
    return eq(sqr(p.y), add(mul(sqr(p.x), p.x), CurveB<F>::get()));   // (written out: through a function shared with keyio.hip.h the kernels come out with other registers)
}

template <class P> GA_HD Fe2<P> check_conj(const Fe2<P>& a) { return {a.c0, neg(a.c1)}; }
template <class P> GA_HD Fe2<P> check_mul_fp(const Fe2<P>& a, const Fe<P>& k) { return {mul(a.c0, k), mul(a.c1, k)}; }
// (x, y, zz, zzz) -> (conj(x) cx, conj(y) cy, conj(zz), conj(zzz)): psi, or psi^3 with its own constants, of a projective point
template <class P>
__device__ __forceinline__ XYZZ<Fe2<P>> check_frobenius(const XYZZ<Fe2<P>>& q, const Fe2<P>& cx, const Fe2<P>& cy) {
    return {mul(check_conj(q.x), cx), mul(check_conj(q.y), cy), check_conj(q.zz), check_conj(q.zzz)};
}
template <class F>
__device__ __forceinline__ bool check_same_point(const XYZZ<F>& a, const XYZZ<F>& b) {
    if (is_inf(a) | is_inf(b)) return is_inf(a) & is_inf(b);
    return eq(mul(a.x, b.zz), mul(b.x, a.zz)) & eq(mul(a.y, b.zzz), mul(b.y, a.zzz));
}

// acc = [S] acc for the compile-time S: one doubling per bit below the top one, one addition per set bit, the same for every lane
template <class F, uint64_t S>
__device__ __forceinline__ void check_seed_mul29(Lazy4<F>& acc, const LdsAcc29<F>& D) {
    D.put(0, acc.x);
    D.put(1, acc.y);
    D.put(2, acc.zz);
    D.put(3, acc.zzz);
    constexpr int TOP = 63 - __builtin_clzll(S);
#pragma unroll 1
    for (int b = TOP - 1; b >= 0; b--) {
        dbl29<F>(acc);
        if ((S >> b) & 1) {
            const Lazy4<F> d{D.get(0), D.get(1), D.get(2), D.get(3)};
            add29<F>(acc, d);
        }
    }
}

// the closing of each identity on reduced values; q = [|x0|]P (BLS12-381 G1: [x0^2]P), not infinity
template <class P>
__device__ __forceinline__ bool check_close_bls_g1(const Affine<Fe<P>>& p, const XYZZ<Fe<P>>& q) {
    return eq(mul(fe_const<P>(P::BETA), q.x), mul(p.x, q.zz)) & eq(q.y, neg(mul(p.y, q.zzz)));
}
template <class P>
__device__ __forceinline__ bool check_close_bls_g2(const Affine<Fe2<P>>& p, const XYZZ<Fe2<P>>& q) {
    const Fe2<P> cx{fe_const<P>(P::PSI_X0), fe_const<P>(P::PSI_X1)}, cy{fe_const<P>(P::PSI_Y0), fe_const<P>(P::PSI_Y1)};
    const Fe2<P> px = mul(check_conj(p.x), cx), py = mul(check_conj(p.y), cy);
    return eq(mul(px, q.zz), q.x) & eq(mul(py, q.zzz), neg(q.y));
}
template <class P>
__device__ __forceinline__ bool check_close_bn_g2(const Affine<Fe2<P>>& p, const XYZZ<Fe2<P>>& q) {
    const Fe2<P> cx{fe_const<P>(P::PSI_X0), fe_const<P>(P::PSI_X1)}, cy{fe_const<P>(P::PSI_Y0), fe_const<P>(P::PSI_Y1)};
    const Fe2<P> c3x{fe_const<P>(P::PSI3_X0), fe_const<P>(P::PSI3_X1)}, c3y{fe_const<P>(P::PSI3_Y0), fe_const<P>(P::PSI3_Y1)};
    XYZZ<Fe2<P>> lhs = madd(q, p);
    lhs = add(lhs, check_frobenius(q, cx, cy));
    const XYZZ<Fe2<P>> q2{check_mul_fp(q.x, fe_const<P>(P::PSI2_X)), check_mul_fp(q.y, fe_const<P>(P::PSI2_Y)), q.zz, q.zzz};
    lhs = add(lhs, q2);
    return check_same_point(lhs, check_frobenius(dbl(q), c3x, c3y));
}

// what a lane reports: its status byte, and for a bad point the call's counters
__device__ __forceinline__ void check_report(uint8_t* __restrict__ status, uint32_t i, uint64_t base, int st, CheckCounters* __restrict__ cnt) {
    status[i] = (uint8_t)st;
    if (st == GA_POINT_OK) return;
    atomicAdd(st == GA_POINT_OFF_CURVE ? &cnt->off : &cnt->outside, 1ull);
    atomicMax(st == GA_POINT_OFF_CURVE ? &cnt->first_off_inv : &cnt->first_outside_inv, ~(uint32_t)(base + i));
}

// 0 / 1: decided (infinity, off the curve, nothing more to test); -1: the ladder
template <class F>
__device__ __forceinline__ int check_classify(const Affine<F>& P, int curve_only, bool has_ladder) {
    // (0,0) first: it is reduced, and gnark-crypto's IsOnCurve / IsInSubGroup accept it
    if (is_inf(P)) return GA_POINT_OK;
    if (!check_on_curve<F>(P)) return GA_POINT_OFF_CURVE;
    return (curve_only || !has_ladder) ? GA_POINT_OK : -1;
}

template <class F>
__global__ void __launch_bounds__(Table29<F>::THREADS, CheckLadder<F>::MIN_WAVES)
check_points_kernel(const Affine<F>* __restrict__ points, uint32_t n, uint64_t base, int curve_only, uint8_t* __restrict__ status,
                    CheckCounters* __restrict__ cnt, uint32_t* __restrict__ redo, uint32_t* __restrict__ redo_count) {
    constexpr int NW = Lazy<F>::NW;
    constexpr int RULE = CheckRule<F>::RULE;
    constexpr uint64_t SEED = CheckRule<F>::SEED;
    __shared__ uint32_t lds[4 * NW * Table29<F>::THREADS];
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const Affine<F> P = load_pod<Affine<F>>(&points[i]);
        const int decided = check_classify<F>(P, curve_only, RULE != CHECK_RULE_CURVE);
        if (decided >= 0) {
            check_report(status, i, base, decided, cnt);
            continue;
        }
        if constexpr (RULE != CHECK_RULE_CURVE) {
            Lazy4<F> acc = affine_to_lazy4<F>(P);
            const LdsAcc29<F> D(lds + threadIdx.x);
            check_seed_mul29<F, SEED>(acc, D);
            if constexpr (RULE == CHECK_RULE_BLS_G1) check_seed_mul29<F, SEED>(acc, D);
            if (f29_is_zero_mod_p(acc.zz)) {
                redo[atomicAdd(redo_count, 1u)] = i;
                continue;
            }
            const XYZZ<F> q = ec_ntt_to_exact<F>(ec_ntt_pack<F>(acc));
            bool ok;
            if constexpr (RULE == CHECK_RULE_BLS_G1) ok = check_close_bls_g1(P, q);
            else if constexpr (RULE == CHECK_RULE_BLS_G2) ok = check_close_bls_g2(P, q);
            else ok = check_close_bn_g2(P, q);
            check_report(status, i, base, ok ? GA_POINT_OK : GA_POINT_NOT_IN_SUBGROUP, cnt);
        }
    }
}

// the definition: [r - 1]P = -P on the plain ladder (rm1: r - 1, canonical words)
template <class F, class FrP>
__global__ void __launch_bounds__(Table29<F>::THREADS, CheckLadder<F>::NAIVE_MIN_WAVES)
check_points_naive_kernel(const Affine<F>* __restrict__ points, uint32_t n, uint64_t base, int curve_only, const Fe<FrP> rm1, uint8_t* __restrict__ status,
                          CheckCounters* __restrict__ cnt, uint32_t* __restrict__ redo, uint32_t* __restrict__ redo_count) {
    constexpr int NW = Lazy<F>::NW;
    __shared__ uint32_t lds[4 * NW * Table29<F>::THREADS];
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const Affine<F> P = load_pod<Affine<F>>(&points[i]);
        const int decided = check_classify<F>(P, curve_only, true);
        if (decided >= 0) {
            check_report(status, i, base, decided, cnt);
            continue;
        }
        uint32_t k[8];
#pragma unroll
        for (int w = 0; w < 8; w++) k[w] = rm1.l[w];
        Lazy4<F> acc = affine_to_lazy4<F>(P);
        ec_ntt_scalar_mul29<F>(acc, LdsAcc29<F>(lds + threadIdx.x), k);
        if (f29_is_zero_mod_p(acc.zz)) {
            redo[atomicAdd(redo_count, 1u)] = i;
            continue;
        }
        const XYZZ<F> q = ec_ntt_to_exact<F>(ec_ntt_pack<F>(acc));
        const bool ok = eq(q.x, mul(P.x, q.zz)) & eq(q.y, neg(mul(P.y, q.zzz)));
        check_report(status, i, base, ok ? GA_POINT_OK : GA_POINT_NOT_IN_SUBGROUP, cnt);
    }
}

// the flagged lanes of a chunk (curve points, not infinity) with the complete formulas: [r]P = O or not; lane 0 adds their number to
// the call's total (the kernels of a call run one after the other on one stream)
template <class F, class FrP>
__global__ void __launch_bounds__(64)
check_points_exact_kernel(const Affine<F>* __restrict__ points, uint64_t base, const Fe<FrP> r, uint8_t* __restrict__ status, CheckCounters* __restrict__ cnt,
                          const uint32_t* __restrict__ redo, const uint32_t* __restrict__ redo_count) {
    const uint32_t nredo = *redo_count;
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt->redone += nredo;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < nredo; j += gridDim.x * blockDim.x) {
        const uint32_t i = redo[j];
        uint32_t k[8];
#pragma unroll
        for (int w = 0; w < 8; w++) k[w] = r.l[w];
        const XYZZ<F> q = scalar_mul(to_xyzz(load_pod<Affine<F>>(&points[i])), k, 8);
        check_report(status, i, base, is_inf(q) ? GA_POINT_OK : GA_POINT_NOT_IN_SUBGROUP, cnt);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct CheckScratch {
    uint8_t* status = nullptr;      // chunk bytes: the status of a chunk when the caller's is on the host, or NULL
    RedoList redo;                  // header: CheckCounters (8 words), the chunk's count, pad, pad, pad
    uint64_t chunk = 0;
    CheckCounters* counters() const { return (CheckCounters*)redo.words; }
    uint32_t* count() const { return redo.words + 8; }
    uint32_t* list() const { return redo.list; }
};
inline int check_scratch_get(Ctx* ctx, uint64_t n, uint64_t forced_chunk, CheckScratch* s) {
    s->chunk = clamp_chunk(forced_chunk, CHECK_DEFAULT_CHUNK, n);
    if (s->chunk == 0) s->chunk = 1;   // (n = 0: the scratch still exists)
    GA_CHECK(ctx->scratch_get("check_status", (s->chunk + 15) & ~15ull, (void**)&s->status));
    return s->redo.get(ctx, "check_redo", s->chunk, 12);
}

// the counters -> the four words of the ABI, after draining the stream
inline int check_read_counters(const CheckScratch& s, hipStream_t st, uint64_t* out4, int* first_status) {
    CheckCounters h;
    GA_HIP_CHECK(hipMemcpyAsync(&h, s.counters(), sizeof(h), hipMemcpyDeviceToHost, st));
    GA_HIP_CHECK(hipStreamSynchronize(st));
    // (index 2^32 - 1 complements to 0, "none", as well: the counts tell the two apart)
    const uint64_t f_off = h.off ? (uint64_t)(uint32_t)~h.first_off_inv : UINT64_MAX, f_out = h.outside ? (uint64_t)(uint32_t)~h.first_outside_inv : UINT64_MAX;
    out4[0] = h.off;
    out4[1] = h.outside;
    out4[2] = f_off < f_out ? f_off : f_out;
    out4[3] = h.redone;
    if (first_status) *first_status = (h.off | h.outside) == 0 ? GA_POINT_OK : (f_off < f_out ? GA_POINT_OFF_CURVE : GA_POINT_NOT_IN_SUBGROUP);
    return GA_OK;
}

// one chunk: cn points at `src` (device), global index of its first point `base`; status bytes to `st_out` (device)
template <class C, int G>
int check_points_launch(Ctx* ctx, hipStream_t st, const CheckScratch& s, const void* src, uint32_t cn, uint64_t base, int curve_only, int naive,
                        uint8_t* st_out) {
    typedef typename GroupField<C, G>::F F;
    typedef typename C::FrP FrP;
    constexpr unsigned T = Table29<F>::THREADS;
    Fe<FrP> r = fe_zero<FrP>(), rm1;
    for (int w = 0; w < FrP::N; w++) r.l[w] = FrP::MOD[w];
    rm1 = r;
    rm1.l[0] -= 1;   // r is odd
    GA_HIP_CHECK(hipMemsetAsync(s.count(), 0, 16, st));
    StageTimer tm(ctx, "check_ladder");
    const unsigned blocks = capped_grid(cn, T, CHECK_MAX_BLOCKS), exact_blocks = capped_grid(cn, 64, EC_NTT_EXACT_MAX_BLOCKS);
    if (naive)
        hipLaunchKernelGGL((check_points_naive_kernel<F, FrP>), dim3(blocks), dim3(T), 0, st, (const Affine<F>*)src, cn, base, curve_only, rm1, st_out, s.counters(),
                           s.list(), s.count());
    else
        hipLaunchKernelGGL((check_points_kernel<F>), dim3(blocks), dim3(T), 0, st, (const Affine<F>*)src, cn, base, curve_only, st_out, s.counters(), s.list(),
                           s.count());
    hipLaunchKernelGGL((check_points_exact_kernel<F, FrP>), dim3(exact_blocks), dim3(64), 0, st, (const Affine<F>*)src, base, r, st_out, s.counters(),
                       (const uint32_t*)s.list(), (const uint32_t*)s.count());
    GA_KERNEL_CHECK();
    return GA_OK;
}

// naive: GA_CHECK_NAIVE; forced_chunk: GA_CHECK_CHUNK (0 = default)
template <class C, int G>
int check_points_run(Ctx* ctx, const void* points, size_t n, unsigned flags, uint8_t* status, uint64_t* out4, int naive, uint64_t forced_chunk) {
    typedef typename GroupField<C, G>::F F;
    const bool i_dev = (flags & GA_BASES_ON_DEVICE) != 0, o_dev = (flags & GA_RESULT_ON_DEVICE) != 0;
    const int curve_only = (flags & GA_CHECK_CURVE_ONLY) != 0;
    hipStream_t st = ctx->work_stream();

    // the scratch of the whole call first: an allocation failure leaves nothing in flight
    CheckScratch s;
    Affine<F>* io = nullptr;
    GA_CHECK(check_scratch_get(ctx, n, forced_chunk, &s));
    if (!i_dev) GA_CHECK(ctx->scratch_get("check_io", s.chunk * sizeof(Affine<F>), (void**)&io));
    StreamDrain drain{st};

    GA_HIP_CHECK(hipMemsetAsync(s.counters(), 0, sizeof(CheckCounters), st));
    for (uint64_t done = 0; done < n; done += s.chunk) {
        const uint32_t cn = (uint32_t)(n - done < s.chunk ? n - done : s.chunk);
        const Affine<F>* src;
        GA_CHECK(chunk_in(st, i_dev, (const Affine<F>*)points, done, cn, io, &src));
        uint8_t* st_out = (status && o_dev) ? status + done : s.status;
        GA_CHECK((check_points_launch<C, G>(ctx, st, s, src, cn, done, curve_only, naive, st_out)));
        if (status) GA_CHECK(chunk_out(st, o_dev, status, done, cn, s.status));
    }
    GA_CHECK(check_read_counters(s, st, out4, nullptr));   // the one synchronisation of a call with everything on the device
    return GA_OK;
}

// ---- points that already sit on the device: the checked key reads (g16_io.hip.h) ----------------------------------------------------
// Launches only, on `st`: n points at d_points, `base` the index of the first one within its vector (below 2^32); reset starts a
// new tally.  The scratch is always that of a default chunk, so it never moves between the calls of one read.
template <class C, int G>
int check_points_resident(Ctx* ctx, hipStream_t st, const void* d_points, uint64_t n, uint64_t base, int reset, int naive) {
    typedef typename GroupField<C, G>::F F;
    CheckScratch s;
    GA_CHECK(check_scratch_get(ctx, CHECK_DEFAULT_CHUNK, 0, &s));
    if (reset) GA_HIP_CHECK(hipMemsetAsync(s.counters(), 0, sizeof(CheckCounters), st));
    for (uint64_t done = 0; done < n; done += s.chunk) {
        const uint32_t cn = (uint32_t)(n - done < s.chunk ? n - done : s.chunk);
        GA_CHECK((check_points_launch<C, G>(ctx, st, s, (const Affine<F>*)d_points + done, cn, base + done, 0, naive, s.status)));
    }
    return GA_OK;
}
// drains `st` and reads the tally: out4 as ga_check_points', *first_status the failure of the point at out4[2] (GA_POINT_OK if none)
template <class C, int G>
int check_points_tally(Ctx* ctx, hipStream_t st, uint64_t* out4, int* first_status) {
    CheckScratch s;
    GA_CHECK(check_scratch_get(ctx, CHECK_DEFAULT_CHUNK, 0, &s));
    return check_read_counters(s, st, out4, first_status);
}

// what check_points_<curve>_g<k>.hip instantiates
#define GA_INSTANTIATE_CHECK_POINTS(C, G)                                                                            \
    template int check_points_run<C, G>(Ctx*, const void*, size_t, unsigned, uint8_t*, uint64_t*, int, uint64_t);    \
    template int check_points_resident<C, G>(Ctx*, hipStream_t, const void*, uint64_t, uint64_t, int, int);          \
    template int check_points_tally<C, G>(Ctx*, hipStream_t, uint64_t*, int*);

}  // namespace ga

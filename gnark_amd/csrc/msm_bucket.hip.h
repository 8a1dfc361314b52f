// Stage 4 of the MSM pipeline (msm.hip.h): one lane per task sums the task's table entries into a bucket (or partial) sum; and the
// kernels that build what it gathers from -- the window tables of pinned keys, the hat-domain copy of un-pinned bases.
#pragma once
#include "msm_lazy.hip.h"
#include "msm_sort.hip.h"   // MSM_SIGN: the format of the sorted values

namespace ga {

constexpr int GA_ACC29_MINW = 4;      // waves per SIMD requested for the G1 bucket kernel (2 for Fp2 points: 72 KiB of LDS per workgroup)
#ifndef GA_ACC29_FP2_MINW             // (compile-time experiments only: tools/exp/r06_bls_g2_two_waves.sh)
#define GA_ACC29_FP2_MINW 2
#endif

// ---- 4. accumulate over a table in the unpacked ("29-bit limb") format ---------------------------------------------------------
// Table entry = hat(x) | hat(y) as NL limbs each (field29.hip.h), padded to a multiple of 16 bytes; (0,0) = infinity.
// The bucket loop runs entirely in the lazy representation: per mixed addition 10 products of 2*NL^2 MADs + one
// shift/mask per column, limb-wise add/sub with a carry sweep, no unpacking, no conditional subtractions.  The
// exceptional cases of the addition law (doubling, P + (-P), accumulator at infinity) are not branched on: they all
// make ZZ == 0 (mod p) and 0 is absorbing, so ONE exact test when the task ends detects them; such tasks are queued for
// msm_accumulate29_redo_kernel, which repeats them with the complete formulas.
template <class F>
struct Table29 {
    static constexpr int NW = Lazy<F>::NW;                 // 32-bit registers per coordinate once unpacked
    // In HBM a table entry is the hat-domain point with each coordinate packed as an ordinary 32N-bit integer: 64 B
    // (BN254 G1, half a cache line, never straddling), 128 B (BN254 G2, one line), 96 / 192 B for BLS12-381.  Storing the
    // limbs unpacked (80 B for BN254 G1) made every third gather touch two lines: FETCH_SIZE 41 GB per 2^24 MSM.
    static constexpr int WORDS = sizeof(Affine<F>) / 4;
    // workgroup size: the LDS-resident accumulators (4*NW words per lane) must leave room for 2 workgroups per CU.  (Measured and
    // removed -- tools/exp/r04_pruned_knobs.patch brings the build knobs back: 128- / 64-lane workgroups for the 14-limb fields,
    // G1 30.41 / 30.92 / 30.44 ms per 2^24 launch, G2 95.6 at 128 lanes / 108.6 at 64, profiles/r03_v_bls_workgroup_size_ab.txt;
    // the next table entry requested one addition ahead and parked in registers: G2 97.1 -> 95.9 ms on BLS12-381, nothing on the
    // other three kernels, profiles/r04_a_prefetch_ab.txt.)
    static constexpr int THREADS = (4 * NW * 4 * 256 <= 72 * 1024) ? 256 : 128;
    static constexpr int MIN_WAVES = Lazy<F>::FP2 ? GA_ACC29_FP2_MINW : GA_ACC29_MINW;
};

// The lane's XYZZ accumulator lives in LDS, word-major (conflict-free): that is what keeps the G1 kernel at 128 VGPRs and four waves
// per SIMD (the accumulator in registers measured slower in round 3: 15.58 vs 15.04 ms per 2^24 launch, profiles/README.md).
template <class F>
struct LdsAcc29 {
    typedef typename Lazy<F>::T T;
    uint32_t* base;
    __device__ __forceinline__ explicit LdsAcc29(uint32_t* b) : base(b) {}
    static constexpr int NW = Lazy<F>::NW, STRIDE = Table29<F>::THREADS;
    __device__ __forceinline__ T get(int field) const {
        T r;
#pragma unroll
        for (int i = 0; i < NW; i++) Lazy<F>::set_word(r, i, base[(field * NW + i) * STRIDE]);
        return r;
    }
    __device__ __forceinline__ void put(int field, const T& v) const {
#pragma unroll
        for (int i = 0; i < NW; i++) base[(field * NW + i) * STRIDE] = Lazy<F>::word(v, i);
    }
};

template <class F>
__device__ __forceinline__ void load_point29(const uint32_t* __restrict__ table, uint32_t idx, typename Lazy<F>::T& x,
                                             typename Lazy<F>::T& y) {
    Affine<F> a = load_pod<Affine<F>>(table + (uint64_t)idx * Table29<F>::WORDS);
    x = Lazy<F>::unpack(a.x);
    y = Lazy<F>::unpack(a.y);
}

// acc += q in the lazy representation (madd-2008-s).  Subtraction constants and partial reductions come from the bound
// analysis in DESIGN.md ("lazy bounds"): G1 keeps every value < 2^257 (BN254) / 2^385 (BLS12-381) with no reduction at
// all; G2 (Karatsuba doubles the operand bounds) additionally applies f29_partial_reduce to P, R, PPP and X3.
template <class P>
__device__ __forceinline__ void madd29(const LdsAcc29<Fe<P>>& A, const F29<P>& qx, const F29<P>& qy) {
    F29<P> zz = A.get(2);
    F29<P> U2 = f29_mul(qx, zz);
    F29<P> ax = A.get(0);
    F29<P> Pp = f29_sub<8>(U2, ax);
    F29<P> zzz = A.get(3);
    F29<P> S2 = f29_mul(qy, zzz);
    F29<P> ay = A.get(1);
    F29<P> R = f29_sub<8>(S2, ay);
    F29<P> PP = f29_sqr(Pp);
    A.put(2, f29_mul(zz, PP));
    F29<P> PPP = f29_mul(Pp, PP);
    A.put(3, f29_mul(zzz, PPP));
    F29<P> Q = f29_mul(ax, PP);
    // X3 = R^2 - (PPP + 2Q): the sum stays un-normalized (limbs < 3*2^L) and is subtracted with a 4-unit loan: one carry
    // sweep instead of three; t = Q - X3 + 8p also stays raw (limbs < 3*2^L): a 2^31-limb multiplicand keeps the two product
    // columns of f29_mul_sub below 2^64
    F29<P> X3 = f29_sub_wide<4, 4>(f29_sqr(R), f29_add_raw(PPP, f29_add_raw(Q, Q)));
    A.put(0, X3);
    A.put(1, f29_mul_sub<8>(R, f29_sub_raw<8>(Q, X3), ay, PPP));   // Y3 = R*(Q - X3) - Y1*PPP, one reduction
}

template <class P>
__device__ __forceinline__ void madd29(const LdsAcc29<Fe2<P>>& A, const F29x2<P>& qx, const F29x2<P>& qy) {
    typedef F29x2<P> T;
    T zz = A.get(2);
    T U2 = f29_mul(qx, zz);
    T ax = A.get(0);
    T Pp = f29_sub<4>(U2, ax);
    T zzz = A.get(3);
    T S2 = f29_mul(qy, zzz);
    T ay = A.get(1);
    T R = f29_sub<4>(S2, ay);
    T PP = f29_sqr(Pp);
    A.put(2, f29_mul(zz, PP));
    T PPP = f29_mul(Pp, PP);
    A.put(3, f29_mul(zzz, PPP));
    T Q = f29_mul(ax, PP);
    T X3 = f29_partial_reduce(f29_sub_wide<4, 4>(f29_sqr(R), f29_add_raw(PPP, f29_add_raw(Q, Q))));
    A.put(0, X3);
    A.put(1, f29_mul_sub<P::FP2Z_K>(R, f29_sub<8>(Q, X3), ay, PPP));   // Y3 = R*(Q - X3) - Y1*PPP, two reductions instead of four
}

// acc = 2*(qx, qy) for an affine q in the lazy representation (mdbl-2008-s-1, a = 0); qy may be a negated 2p - y.  Bounds
// (tools/lazy_bounds.py check_mdbl): every output stays below the fixed-point bounds of the accumulator coordinates of madd29.
template <class F>
__device__ __forceinline__ void mdbl29(const LdsAcc29<F>& A, const typename Lazy<F>::T& qx, const typename Lazy<F>::T& qy) {
    typedef typename Lazy<F>::T T;
    typedef typename Lazy<F>::Params P;
    const T U = f29_add(qy, qy);
    const T V = f29_sqr(U);
    const T W = f29_mul(U, V);
    const T S = f29_mul(qx, V);
    const T xx = f29_sqr(qx);
    const T M = f29_add(f29_add(xx, xx), xx);
    T X3 = f29_sub<4>(f29_sqr(M), f29_add(S, S));
    if constexpr (Lazy<F>::FP2) X3 = f29_partial_reduce(X3);
    constexpr int KMS = Lazy<F>::FP2 ? P::FP2Z_K : 8;
    A.put(1, f29_mul_sub<KMS>(M, f29_sub<8>(S, X3), W, qy));   // Y3 = M*(S - X3) - W*y
    A.put(0, X3);
    A.put(2, V);
    A.put(3, W);
}

// acc += q with the exceptional cases of the addition law handled: same x and same y -> doubling, same x and opposite y -> the
// accumulator becomes the point at infinity (returns false: the caller restarts it with the next point).  One exact zero test of
// P = X2*ZZ1 - X1 per addition (~80 instructions on top of the ~2400 of madd29); R is only tested when P vanishes.
template <class F>
__device__ __forceinline__ bool madd29_complete(const LdsAcc29<F>& A, const typename Lazy<F>::T& qx, const typename Lazy<F>::T& qy) {
    typedef typename Lazy<F>::T T;
    typedef typename Lazy<F>::Params P;
    constexpr int KS = Lazy<F>::FP2 ? 4 : 8;
    const T Pp = f29_sub<KS>(f29_mul(qx, A.get(2)), A.get(0));
    if (f29_is_zero_mod_p(Pp)) {
        const T R = f29_sub<KS>(f29_mul(qy, A.get(3)), A.get(1));
        if (!f29_is_zero_mod_p(R)) return false;
        mdbl29<F>(A, qx, qy);
        return true;
    }
    madd29<P>(A, qx, qy);   // (recomputes P: the common path stays the code the bound analysis covers)
    return true;
}

// one task = the sorted pairs [start, end): its sum into the lane's LDS accumulator; returns whether the sum is a finite point
template <class F, bool COMPLETE>
__device__ __forceinline__ bool accumulate_task29(const LdsAcc29<F>& A, const uint32_t* __restrict__ table, const uint32_t* __restrict__ vals,
                                                  uint32_t start, uint32_t end) {
    typedef typename Lazy<F>::T T;
    typedef typename Lazy<F>::Params P;
    const T one = Lazy<F>::from_mem(FieldTraits<F>::one());
    bool have = false;
    uint32_t v = vals[start];
    uint32_t vn = v;
    for (uint32_t p = start; p < end; p++) {
        T qx, qy;
        vn = p + 1 < end ? vals[p + 1] : v;
        load_point29<F>(table, v & ~MSM_SIGN, qx, qy);
        if (!(f29_is_zero_limbs(qx) & f29_is_zero_limbs(qy))) {   // (0,0) = infinity: skip
            if (v & MSM_SIGN) qy = f29_sub<2>(Lazy<F>::from_mem(FieldTraits<F>::zero()), qy);   // 2p - y
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
        v = vn;
    }
    return have;
}

// the task's sum out of the LDS accumulator: false when an exceptional addition slipped through (ZZ == 0 mod p)
template <class F>
__device__ __forceinline__ bool store_task29(const LdsAcc29<F>& A, bool have, XYZZ<F>* __restrict__ dst) {
    XYZZ<F> acc = xyzz_inf<F>();
    if (have) {
        F zz = Lazy<F>::to_mem(A.get(2));
        if (is_zero(zz)) return false;
        acc.x = Lazy<F>::to_mem(A.get(0));
        acc.y = Lazy<F>::to_mem(A.get(1));
        acc.zz = zz;
        acc.zzz = Lazy<F>::to_mem(A.get(3));
    }
    store_pod(dst, acc);
    return true;
}

// COMPLETE = false: the fast loop (exceptional additions make ZZ == 0 and flag the task); true: the same loop with the exceptional
// cases handled in place -- used directly on tables that turned out degenerate (a DummySetup key: every base the same point).
// Multi-table pass (the Groth16 witness MSMs A, B1, K: ONE scalar vector, k wire-indexed tables of the same shape): blockIdx.y is
// the table; its sums live in the table's own slice of [k x nb bucket sums | k x max_tasks partial sums] and its flagged tasks in its
// own redo lists.  A single-table launch is the case k = 1, y = 0 of the same arithmetic.
struct MsmTables {
    const uint32_t* t[4];
    uint32_t k, nb, max_tasks;
};
__device__ __forceinline__ uint32_t msm_multi_dest(const MsmTables& mt, uint32_t dest) {
    return dest < mt.nb ? dest + blockIdx.y * mt.nb : dest + (mt.k - 1) * mt.nb + blockIdx.y * mt.max_tasks;
}

#ifdef GA_ACC29_NUM_VGPR   // (compile-time experiment: FORCE that many waves per SIMD on the bucket kernel -- the allocator must spill to get there; tools/exp/r06_bls_g2_two_waves.sh)
#define GA_ACC29_VGPR_ATTR __attribute__((amdgpu_waves_per_eu(GA_ACC29_NUM_VGPR, GA_ACC29_NUM_VGPR)))
#else
#define GA_ACC29_VGPR_ATTR
#endif
template <class F, bool COMPLETE>
__global__ void __launch_bounds__(Table29<F>::THREADS, Table29<F>::MIN_WAVES) GA_ACC29_VGPR_ATTR
msm_accumulate29_kernel(const MsmTables mt, const uint32_t* __restrict__ vals,
                        const uint32_t* __restrict__ task_start, const uint32_t* __restrict__ task_qkey_sorted,
                        const uint32_t* __restrict__ task_key_by_tid, const uint32_t* __restrict__ task_perm, uint32_t max_tasks, uint32_t seg,
                        const uint32_t* __restrict__ task_dest, XYZZ<F>* __restrict__ sums, uint32_t* __restrict__ redo_list,
                        uint32_t* __restrict__ redo_count) {
    constexpr int NW = Lazy<F>::NW;
    __shared__ uint32_t lds[4 * NW * Table29<F>::THREADS];
    // (Round 3 measured two ways of making room for kernels of the partner lane beside this one -- which fills 144 of the 160 KB
    // of LDS of a CU: the accumulator in registers instead of LDS (15.58 vs 15.04 ms, slower) and a cap of 3 resident waves per
    // SIMD through the register allocation (proof time unchanged, 139.4 vs 139.9 ms).  Neither stays.  Round 4: a resident grid
    // striding over the task list instead of one task per lane is slower on all four kernels, tools/exp/r04_resident_bucket_grid.patch,
    // profiles/r04_e_resident_bucket_grid_ab.txt.)
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= max_tasks) return;
    if (task_qkey_sorted[t] == 0xFFFFFFFFu) return;   // padding slot of the task list
    const uint32_t tid = task_perm[t];
    const uint32_t key = task_key_by_tid[tid];
    const uint32_t start = task_start[tid];
    LdsAcc29<F> A(lds + threadIdx.x);
    const bool have = accumulate_task29<F, COMPLETE>(A, mt.t[blockIdx.y], vals, start, start + (seg - key));
    if (!store_task29<F>(A, have, &sums[msm_multi_dest(mt, task_dest[tid])]))   // redo it
        redo_list[(uint64_t)blockIdx.y * (mt.max_tasks + 2) + atomicAdd(redo_count + 2 * blockIdx.y, 1u)] = tid;
}

// second chance for the tasks the fast loop flagged: the complete lazy loop over the redo list (grid-stride); what even that
// cannot finish (a base of order 2, never on these curves) goes to the exact kernel below through a second list
template <class F>
__global__ void __launch_bounds__(Table29<F>::THREADS, Table29<F>::MIN_WAVES)
msm_accumulate29_retry_kernel(const MsmTables mt, const uint32_t* __restrict__ vals,
                              const uint32_t* __restrict__ task_start, const uint32_t* __restrict__ task_key_by_tid, uint32_t seg,
                              const uint32_t* __restrict__ redo_list, const uint32_t* __restrict__ redo_count,
                              const uint32_t* __restrict__ task_dest, XYZZ<F>* __restrict__ sums, uint32_t* __restrict__ redo2_list,
                              uint32_t* __restrict__ redo2_count) {
    constexpr int NW = Lazy<F>::NW;
    __shared__ uint32_t lds[4 * NW * Table29<F>::THREADS];
    // (the lists and counters of table y: see msm_accumulate29_kernel)
    redo_list += (uint64_t)blockIdx.y * (mt.max_tasks + 2);
    redo2_list += (uint64_t)blockIdx.y * (mt.max_tasks + 2);
    const uint32_t nredo = redo_count[2 * blockIdx.y];
    LdsAcc29<F> A(lds + threadIdx.x);
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < nredo; r += gridDim.x * blockDim.x) {
        const uint32_t tid = redo_list[r];
        const uint32_t start = task_start[tid];
        const bool have = accumulate_task29<F, true>(A, mt.t[blockIdx.y], vals, start, start + (seg - task_key_by_tid[tid]));
        if (!store_task29<F>(A, have, &sums[msm_multi_dest(mt, task_dest[tid])])) redo2_list[atomicAdd(redo2_count + 2 * blockIdx.y, 1u)] = tid;
    }
}

// exact re-run of the tasks the lazy kernel flagged (complete formulas; table points converted back to gnark's form)
template <class F>
__global__ void __launch_bounds__(64)
msm_accumulate29_redo_kernel(const MsmTables mt, const uint32_t* __restrict__ vals,
                             const uint32_t* __restrict__ task_start, const uint32_t* __restrict__ task_key_by_tid,
                             uint32_t seg, const uint32_t* __restrict__ redo_list, const uint32_t* __restrict__ redo_count,
                             const uint32_t* __restrict__ task_dest, XYZZ<F>* __restrict__ sums) {
    typedef typename Lazy<F>::T T;
    redo_list += (uint64_t)blockIdx.y * (mt.max_tasks + 2);
    const uint32_t nredo = redo_count[2 * blockIdx.y];
    const uint32_t* __restrict__ table = mt.t[blockIdx.y];
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < nredo; r += gridDim.x * blockDim.x) {
        const uint32_t tid = redo_list[r];
        const uint32_t start = task_start[tid];
        const uint32_t end = start + (seg - task_key_by_tid[tid]);
        XYZZ<F> acc = xyzz_inf<F>();
        for (uint32_t p = start; p < end; p++) {
            const uint32_t v = vals[p];
            T qx, qy;
            load_point29<F>(table, v & ~MSM_SIGN, qx, qy);
            Affine<F> q{Lazy<F>::to_mem(qx), Lazy<F>::to_mem(qy)};
            if (v & MSM_SIGN) q.y = neg(q.y);
            acc = madd(acc, q);
        }
        store_pod(&sums[msm_multi_dest(mt, task_dest[tid])], acc);
    }
}

// ---- precomputed tables (pinned keys): table29[w*n + i] = [2^(c*w)] P_i in the packed hat format ------------------------------
// With 288 GB of HBM a pinned key can afford windows x its size: all windows then share one bucket set (one
// reduction instead of `windows`, no Horner) and c can grow to 23 => 12 instead of 14 window passes over the scalars.
// (ICICLE exposes the same idea as MSMConfig.PrecomputeFactor, icicle.go:507-525.)  The doubling chain is dbl29 (msm_lazy.hip.h).
// A lane carries TableBatch<F>::K points through the doubling chain together, in the lazy representation (the chain is 22 doublings
// per window step: 9 products each, no reductions in between), and brings them back to affine with ONE field inversion per window
// step (Montgomery's trick on zz*zzz; lanes of a wave cannot share one -- SIMD: 64 inversions cost what one costs -- so the batch
// is inside the lane).  The affine coordinates leave the lane as canonical packed hat-domain words: the table's storage format.
// History (2^22 points, kernel time): exact arithmetic, one point per lane 0.248 s (BN254 G1) / 0.835 s (BLS12-381 G1) / 0.627 s
// (BN254 G2); exact arithmetic with 8 / 2 points per lane 0.158 / 0.392 / 0.594 s; this version: see profiles/r02_h notes.
template <class F> struct TableBatch { static constexpr int K = BaseFieldOf<F>::IS_FP ? (BaseFieldOf<F>::P::N <= 8 ? 4 : 2) : (BaseFieldOf<F>::P::N <= 8 ? 2 : 1); };

template <class F>
__global__ void __launch_bounds__(64)
msm_table29_kernel(const Affine<F>* __restrict__ bases, uint64_t n, int c, int nwin, uint32_t* __restrict__ table) {
    typedef typename Lazy<F>::T T;
    constexpr int K = TableBatch<F>::K;
    const uint64_t lanes = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n) return;   // point q of a lane is gid + q*lanes: nothing to do when even q = 0 is out of range
    const T one = Lazy<F>::from_mem(FieldTraits<F>::one());
    Lazy4<F> p[K];
    bool live[K], inf[K];
#pragma unroll
    for (int q = 0; q < K; q++) {
        const uint64_t i = gid + q * lanes;
        live[q] = i < n;
        Affine<F> a = live[q] ? load_pod<Affine<F>>(&bases[i]) : Affine<F>{FieldTraits<F>::zero(), FieldTraits<F>::zero()};
        inf[q] = is_inf(a);
        p[q].x = Lazy<F>::from_mem(a.x);
        p[q].y = Lazy<F>::from_mem(a.y);
        p[q].zz = one;
        p[q].zzz = one;
    }
    for (int w = 0; w < nwin; w++) {
        if (w > 0) {
#pragma unroll
            for (int q = 0; q < K; q++)
                if (!inf[q])
                    for (int k = 0; k < c; k++) dbl29<F>(p[q]);
            // batch to affine: t_q = zz_q * zzz_q (1 for a point at infinity, which stays (0,0)), one inversion of their product
            T t[K], pre[K];
#pragma unroll
            for (int q = 0; q < K; q++) {
                t[q] = inf[q] ? one : f29_mul(p[q].zz, p[q].zzz);
                pre[q] = q == 0 ? t[0] : f29_mul(pre[q - 1], t[q]);
            }
            T run = f29_inv(pre[K - 1]);
#pragma unroll
            for (int q = K - 1; q >= 0; q--) {
                const T it = q > 0 ? f29_mul(run, pre[q - 1]) : run;   // 1 / t_q
                if (q > 0) run = f29_mul(run, t[q]);
                if (!inf[q]) {
                    p[q].x = f29_mul(p[q].x, f29_mul(it, p[q].zzz));   // X / zz
                    p[q].y = f29_mul(p[q].y, f29_mul(it, p[q].zz));    // Y / zzz
                    p[q].zz = one;
                    p[q].zzz = one;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < K; q++) {
            if (!live[q]) continue;
            Affine<F> h{FieldTraits<F>::zero(), FieldTraits<F>::zero()};
            if (!inf[q]) {
                h.x = f29_pack_hat(p[q].x);
                h.y = f29_pack_hat(p[q].y);
                // restart the chain from the canonical coordinates: keeps the doublings' inputs at their smallest
                p[q].x = Lazy<F>::unpack(h.x);
                p[q].y = Lazy<F>::unpack(h.y);
            }
            store_pod(table + ((uint64_t)w * n + gid + q * lanes) * Table29<F>::WORDS, h);
        }
    }
}

// Un-pinned bases -> the packed hat format the bucket kernel gathers (a one-window "table"): S modular doublings per coordinate,
// one point per lane.  (Round 1-4 ran msm_table29_kernel with a single window for this -- a kernel shaped for chains of doublings,
// one wave per block: 83 us for 2^20 points, 1.3 ms for 2^24, of an HBM-bound conversion.)
template <class F>
__global__ void __launch_bounds__(256)
msm_hat_bases_kernel(const Affine<F>* __restrict__ bases, uint64_t n, uint32_t* __restrict__ hat) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine<F> a = load_pod<Affine<F>>(&bases[i]);
    if (!is_inf(a)) {   // (0,0) = infinity stays (0,0): the bucket kernel skips it
        if constexpr (BaseFieldOf<F>::IS_FP) {
            a.x = f29_hat_packed(a.x);
            a.y = f29_hat_packed(a.y);
        } else {
            a.x = {f29_hat_packed(a.x.c0), f29_hat_packed(a.x.c1)};
            a.y = {f29_hat_packed(a.y.c0), f29_hat_packed(a.y.c1)};
        }
    }
    store_pod(hat + i * Table29<F>::WORDS, a);
}

// ---- host: the bucket pass -----------------------------------------------------------------------------------------------------
// The count of flagged tasks travels back asynchronously -- into the lane's pinned words, so that the host keeps launching the merge
// and reduction kernels while the bucket kernel runs (a stack variable, pageable, made that copy a host-side wait for the bucket
// kernel and every launch after it start from an empty queue).  msm_accumulate_reduce holds ONE of these from before the bucket pass
// to its return: every return path, the error returns of every later stage included, leaves with that copy finished.
struct PendingRead {
    hipStream_t st;
    uint32_t stack = 0;
    uint32_t* h;   // per table: [2 i] = tasks the fast loop flagged; without pinned words, table 0's count only
    bool pending = false;
    explicit PendingRead(Ctx* ctx) : st(ctx->work_stream()), h(ctx->pinned_words()) {
        if (!h) h = &stack;
        *h = 0;
    }
    PendingRead(const PendingRead&) = delete;
    ~PendingRead() {
        if (pending) hipStreamSynchronize(st);
    }
    bool pinned() const { return h != &stack; }
};

// Stage 4 on the stream: the fast lazy loop, then the tasks it flagged (an exceptional addition: equal or opposite points met) once
// more with the complete lazy loop, then whatever is left with the exact kernel; last the asynchronous read of the flag counts into
// `read`.  A table on which most tasks were flagged (a DummySetup key: every base the same point) is remembered
// (msm_note_degenerate) and gets the complete loop directly from then on.  *sums: one array [nb bucket sums | max_tasks partial
// sums], tasks write at task_dest (see msm_task_list_kernel); a multi-table pass: [ntab x nb | ntab x max_tasks], so that the bucket
// sums of the tables are the consecutive sets the reduction expects.
template <class F>
int msm_bucket_pass(Ctx* ctx, const void* d_bases, const MsmPrepared& P, const void* const* tables, int ntab, hipStream_t st,
                    PendingRead& read, XYZZ<F>** sums) {
    XYZZ<F>* bsum;
    uint32_t *redo_list, *redo_count, *redo2_list;
    GA_CHECK(ctx->scratch_get("msm_bsum_partial", (uint64_t)ntab * ((uint64_t)P.nb + P.max_tasks) * sizeof(XYZZ<F>), (void**)&bsum));
    GA_CHECK(ctx->scratch_get("msm_redo", (uint64_t)ntab * (P.max_tasks + 2) * 4, (void**)&redo_list));
    GA_CHECK(ctx->scratch_get("msm_redo2", (uint64_t)ntab * (P.max_tasks + 2) * 4, (void**)&redo2_list));
    GA_CHECK(ctx->scratch_get("msm_redo_count", 256, (void**)&redo_count));   // per table: [0] flagged by the first loop, [1] by the retry
    *sums = bsum;
    GA_HIP_CHECK(hipMemsetAsync(redo_count, 0, 8 * ntab, st));
    StageTimer tm(ctx, "msm_accumulate");
    const uint32_t* acc_table = (const uint32_t*)d_bases;
    if (!P.table) {
        // raw (not precomputed) bases: one conversion pass to the packed hat-domain format (a one-window "table"), then the
        // same lazy bucket kernel as the table path (an exact packed-arithmetic kernel cost ~1.5x more per addition: dropped)
        uint32_t* hat;
        GA_CHECK(ctx->scratch_get("msm_hat_bases", (uint64_t)P.n * sizeof(Affine<F>) + 256, (void**)&hat));
        hipLaunchKernelGGL((msm_hat_bases_kernel<F>), dim3((unsigned)((P.n + 255) / 256)), dim3(256), 0, st, (const Affine<F>*)d_bases,
                           (uint64_t)P.n, hat);
        acc_table = hat;
    }
    constexpr unsigned AT = Table29<F>::THREADS;
    const dim3 grid((unsigned)((P.max_tasks + AT - 1) / AT), (unsigned)ntab), redo_grid(1024, (unsigned)ntab);
    MsmTables mt;
    mt.k = (uint32_t)ntab;
    mt.nb = P.nb;
    mt.max_tasks = (uint32_t)P.max_tasks;
    for (int i = 0; i < 4; i++) mt.t[i] = ntab > 1 ? (const uint32_t*)tables[i < ntab ? i : 0] : acc_table;
    // what every bucket kernel takes of the task list
    const uint32_t *vals = P.vals, *start = P.task_start, *qkey = P.task_key, *key = P.task_key_by_id, *perm = P.task_perm, *dest = P.task_dest;
    const uint32_t seg = P.seg;
    auto exact_redo = [&](const uint32_t* list, const uint32_t* count) {
        hipLaunchKernelGGL((msm_accumulate29_redo_kernel<F>), redo_grid, dim3(64), 0, st, mt, vals, start, key, seg, list, count, dest, bsum);
    };
    // (a multi-table pass is only started on tables none of which is known as degenerate: groth16.hip witness_msms)
    if (ntab == 1 && P.table && !ctx->tun.msm_exact_redo && ctx->is_degenerate(d_bases))
        hipLaunchKernelGGL((msm_accumulate29_kernel<F, true>), grid, dim3(AT), 0, st, mt, vals, start, qkey, key, perm, (uint32_t)P.max_tasks, seg,
                           dest, bsum, redo2_list, redo_count + 1);
    else
        hipLaunchKernelGGL((msm_accumulate29_kernel<F, false>), grid, dim3(AT), 0, st, mt, vals, start, qkey, key, perm, (uint32_t)P.max_tasks, seg,
                           dest, bsum, redo_list, redo_count);
    if (!ctx->tun.msm_exact_redo)   // (GA_MSM_EXACT_REDO=1: tests send the flagged tasks straight to the exact kernel below)
        hipLaunchKernelGGL((msm_accumulate29_retry_kernel<F>), dim3(2048, (unsigned)ntab), dim3(AT), 0, st, mt, vals, start, key, seg,
                           (const uint32_t*)redo_list, (const uint32_t*)redo_count, dest, bsum, redo2_list, redo_count + 1);
    else
        exact_redo(redo_list, redo_count);
    exact_redo(redo2_list, redo_count + 1);
    GA_KERNEL_CHECK();
    // read after the stream's final synchronisation (msm_accumulate_reduce)
    GA_HIP_CHECK(hipMemcpyAsync(read.h, redo_count, read.pinned() ? 8 * (size_t)ntab : 4, hipMemcpyDeviceToHost, st));
    read.pending = true;
    return GA_OK;
}

// after the stream's synchronisation: remember the tables on which the fast loop flagged more than a quarter of the tasks
inline void msm_note_degenerate(Ctx* ctx, const MsmPrepared& P, const void* d_bases, const void* const* tables, int ntab, const PendingRead& read) {
    if (!P.table) return;
    if (ntab == 1) {
        if ((uint64_t)*read.h * 4 > P.max_tasks) ctx->mark_degenerate(d_bases);
    } else if (read.pinned()) {
        for (int i = 0; i < ntab; i++)
            if ((uint64_t)read.h[2 * i] * 4 > P.max_tasks) ctx->mark_degenerate(tables[i]);
    }
}

}  // namespace ga

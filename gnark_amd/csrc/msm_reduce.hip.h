// Stages 5 and 6 of the MSM pipeline (msm.hip.h): partial sums -> one sum per bucket (merge), then sum_k k*B_k per bucket set (window
// reduction, exact or lazy) down to a few rows per set, and the host combines that finish them.
#pragma once
#include <vector>

#include "msm_lazy.hip.h"

namespace ga {

constexpr int MSM_HOT_TASKS = 16;     // buckets with more partials than this go to the wave-parallel merge
constexpr uint32_t MSM_VHOT_TASKS = 512;   // ... and with more than this, to the two-stage merge over MSM_VHOT_SPLIT blocks per bucket
constexpr uint32_t MSM_VHOT_SPLIT = 64;
constexpr int MSM_GROUP = 32;         // buckets per running-sum group in the window reduction

// ---- 5. merge partials ----------------------------------------------------------------------------
// hot buckets (17..512 partial sums): one block per bucket
template <class F>
__global__ void __launch_bounds__(64)
msm_hot_kernel(const XYZZ<F>* __restrict__ partial, const uint32_t* __restrict__ task_off,
               const uint32_t* __restrict__ hot_list, const uint32_t* __restrict__ hot_count, XYZZ<F>* __restrict__ bsum,
               uint32_t bsum_stride, uint32_t part_stride) {
    __shared__ LazyPt<F> sh[64];
    __shared__ XYZZ<F> shx[64];
    __shared__ uint32_t bad;
    partial += (uint64_t)blockIdx.y * part_stride;   // (multi-table pass: table y's slices; the lists are the same for every table)
    bsum += (uint64_t)blockIdx.y * bsum_stride;
    const uint32_t nh = *hot_count;
    for (uint32_t h = blockIdx.x; h < nh; h += gridDim.x) {
        const uint32_t b = hot_list[h];
        const uint32_t t0 = task_off[b], t1 = task_off[b + 1];
        block_sum29<F>(t1 - t0, [&](uint32_t i) { return &partial[t0 + i]; }, &bsum[b], sh, shx, &bad);
    }
}

// Very hot buckets (thousands of partial sums: the digit-1 bucket of a boolean-heavy witness): stage 1 gives each of
// MSM_VHOT_SPLIT blocks a contiguous share of the bucket's partials (64 lanes strided + LDS tree), stage 2 sums the
// MSM_VHOT_SPLIT block results of a bucket.  One block per bucket (msm_hot_kernel) would add n/2/seg/64 partials serially per lane:
// measured 4.1 ms (G1) / 16.3 ms (G2) of merge at 2^24 with half the scalars equal to one.
template <class F>
__global__ void __launch_bounds__(64)
msm_vhot_stage1_kernel(const XYZZ<F>* __restrict__ partial, const uint32_t* __restrict__ task_off, const uint32_t* __restrict__ vhot_list,
                       const uint32_t* __restrict__ vhot_count, XYZZ<F>* __restrict__ vtmp, uint32_t part_stride, uint32_t vtmp_stride) {
    __shared__ LazyPt<F> sh[64];
    __shared__ XYZZ<F> shx[64];
    __shared__ uint32_t bad;
    partial += (uint64_t)blockIdx.y * part_stride;
    vtmp += (uint64_t)blockIdx.y * vtmp_stride;
    const uint32_t items = *vhot_count * MSM_VHOT_SPLIT;
    for (uint32_t id = blockIdx.x; id < items; id += gridDim.x) {
        const uint32_t h = id / MSM_VHOT_SPLIT, part = id % MSM_VHOT_SPLIT;
        const uint32_t b = vhot_list[h];
        const uint32_t t0 = task_off[b], t1 = task_off[b + 1];
        const uint32_t per = (t1 - t0 + MSM_VHOT_SPLIT - 1) / MSM_VHOT_SPLIT;
        const uint32_t lo = t0 + part * per < t1 ? t0 + part * per : t1;
        const uint32_t hi = lo + per < t1 ? lo + per : t1;
        block_sum29<F>(hi - lo, [&](uint32_t i) { return &partial[lo + i]; }, &vtmp[id], sh, shx, &bad);
    }
}
template <class F>
__global__ void __launch_bounds__(64)
msm_vhot_stage2_kernel(const XYZZ<F>* __restrict__ vtmp, const uint32_t* __restrict__ vhot_list, const uint32_t* __restrict__ vhot_count,
                       XYZZ<F>* __restrict__ bsum, uint32_t bsum_stride, uint32_t vtmp_stride) {
    static_assert(MSM_VHOT_SPLIT == 64, "one partial result per lane");
    __shared__ LazyPt<F> sh[64];
    __shared__ XYZZ<F> shx[64];
    __shared__ uint32_t bad;
    vtmp += (uint64_t)blockIdx.y * vtmp_stride;
    bsum += (uint64_t)blockIdx.y * bsum_stride;
    const uint32_t nv = *vhot_count;
    for (uint32_t h = blockIdx.x; h < nv; h += gridDim.x)
        block_sum29<F>(MSM_VHOT_SPLIT, [&](uint32_t i) { return &vtmp[h * MSM_VHOT_SPLIT + i]; }, &bsum[vhot_list[h]], sh, shx, &bad);
}

// one lane per bucket: nothing to do for single-task buckets, a serial sum of the 2..16 partial sums (lazy representation: the lane
// is latency-bound on dependent additions; exact re-run by the same lane in the exceptional case), the hot lists for the rest
template <class F>
__global__ void msm_merge_kernel(const XYZZ<F>* __restrict__ partial, const uint32_t* __restrict__ task_off, uint32_t nb,
                                 XYZZ<F>* __restrict__ bsum, uint32_t* __restrict__ hot_list, uint32_t* __restrict__ hot_count,
                                 uint32_t* __restrict__ vhot_list, uint32_t* __restrict__ vhot_count, uint32_t part_stride) {
    uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    // multi-table pass: table y's slices; which buckets are hot depends on the task list alone, so table 0's blocks write the lists
    partial += (uint64_t)blockIdx.y * part_stride;
    bsum += (uint64_t)blockIdx.y * nb;
    uint32_t t0 = task_off[b], t1 = task_off[b + 1];
    uint32_t nt = t1 - t0;
    if (nt == 1) return;   // its only task wrote bsum[b] directly (task_dest)
    if (nt > MSM_VHOT_TASKS) {
        if (blockIdx.y == 0) vhot_list[atomicAdd(vhot_count, 1u)] = b;
        return;
    }
    if (nt > MSM_HOT_TASKS) {
        if (blockIdx.y == 0) hot_list[atomicAdd(hot_count, 1u)] = b;
        return;
    }
    XYZZ<F> out = xyzz_inf<F>();
    bool exact = true;
    // (measured: the lazy sum pays for the 254-bit field -- merge 0.24 -> 0.17 ms G1 -- and loses for the 381-bit one, where the
    // eight conversions of a 14-limb point outweigh ten shorter additions: 0.23 -> 0.27 ms)
    if constexpr (BaseFieldOf<F>::P::N <= 8) {
        LazyPt<F> acc;
        acc.inf = 1;
        for (uint32_t t = t0; t < t1; t++) lazy_acc<F>(acc, load_pod<XYZZ<F>>(&partial[t]));
        exact = false;
        if (!acc.inf) {
            out.zz = Lazy<F>::to_mem(acc.v.zz);
            exact = is_zero(out.zz);   // an exceptional addition: once more with the complete formulas
            out.x = Lazy<F>::to_mem(acc.v.x);
            out.y = Lazy<F>::to_mem(acc.v.y);
            out.zzz = Lazy<F>::to_mem(acc.v.zzz);
        }
    }
    if (exact) {
        out = xyzz_inf<F>();
        for (uint32_t t = t0; t < t1; t++) out = add(out, load_pod<XYZZ<F>>(&partial[t]));
    }
    store_pod(&bsum[b], out);
}

// ---- 6. window reduction ----------------------------------------------------------------------------
// group g of window w covers digits k in [g*m+1, (g+1)*m]; out = sum_k k*B_k over the group
template <class F>
__global__ void __launch_bounds__(64)
msm_reduce_groups_kernel(const XYZZ<F>* __restrict__ bsum, uint32_t half, uint32_t m, uint32_t groups_per_win,
                         uint32_t total_groups, XYZZ<F>* __restrict__ gsum) {
    uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total_groups) return;
    uint32_t w = gid / groups_per_win, g = gid % groups_per_win;
    const XYZZ<F>* B = bsum + (uint64_t)w * half + (uint64_t)g * m;   // B[j] = bucket of digit g*m + j + 1
    XYZZ<F> running = xyzz_inf<F>(), local = xyzz_inf<F>();
    for (int j = (int)m - 1; j >= 0; j--) {
        running = add(running, load_pod<XYZZ<F>>(&B[j]));
        local = add(local, running);
    }
    uint32_t base = g * m;
    if (base != 0) {
        // local += base * running
        XYZZ<F> r = xyzz_inf<F>();
        int top = 31 - __clz(base);
        for (int bit = top; bit >= 0; bit--) {
            r = dbl(r);
            if ((base >> bit) & 1) r = add(r, running);
        }
        local = add(local, r);
    }
    store_pod(&gsum[gid], local);
}

// ---- the same pass in the lazy representation (add29, msm_lazy.hip.h) -----------------------------------------------------------
// lsum[g] = sum_j (j+1)*B_j and rsum[g] = sum_j B_j over the m buckets of group g (no scalar multiplication: the term
// sum_g (g*m)*rsum[g] is assembled from per-bit tree sums, msm_bit_partial_kernel).  Groups in which an exceptional addition
// occurred (e.g. local + running when they are the same point because a bucket was empty) are appended to redo_list.
template <class F>
__global__ void __launch_bounds__(64)
msm_reduce_groups29_kernel(const XYZZ<F>* __restrict__ bsum, uint32_t half, uint32_t m, uint32_t groups_per_win,
                           uint32_t total_groups, XYZZ<F>* __restrict__ lsum, XYZZ<F>* __restrict__ rsum,
                           uint32_t* __restrict__ redo_list, uint32_t* __restrict__ redo_count) {
    uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total_groups) return;
    uint32_t w = gid / groups_per_win, g = gid % groups_per_win;
    const XYZZ<F>* B = bsum + (uint64_t)w * half + (uint64_t)g * m;   // B[j] = bucket of digit g*m + j + 1
    Lazy4<F> running, local;
    bool r_inf = true, l_inf = true;
    for (int j = (int)m - 1; j >= 0; j--) {
        XYZZ<F> b = load_pod<XYZZ<F>>(&B[j]);
        if (!is_inf(b)) {
            Lazy4<F> lb = lazy4_from_mem<F>(b);
            if (r_inf) {
                running = lb;
                r_inf = false;
            } else {
                add29<F>(running, lb);
            }
        }
        if (!r_inf) {
            if (l_inf) {
                local = running;
                l_inf = false;
            } else {
                add29<F>(local, running);
            }
        }
    }
    XYZZ<F> lo = xyzz_inf<F>(), ro = xyzz_inf<F>();
    bool bad = false;
    if (!r_inf) {
        ro.zz = Lazy<F>::to_mem(running.zz);
        lo.zz = Lazy<F>::to_mem(local.zz);
        bad = is_zero(ro.zz) | is_zero(lo.zz);
        ro.x = Lazy<F>::to_mem(running.x);
        ro.y = Lazy<F>::to_mem(running.y);
        ro.zzz = Lazy<F>::to_mem(running.zzz);
        lo.x = Lazy<F>::to_mem(local.x);
        lo.y = Lazy<F>::to_mem(local.y);
        lo.zzz = Lazy<F>::to_mem(local.zzz);
    }
    if (bad) {
        redo_list[atomicAdd(redo_count, 1u)] = gid;
        return;
    }
    store_pod(&lsum[gid], lo);
    store_pod(&rsum[gid], ro);
}

// exact re-run (complete formulas) of the groups the lazy kernel flagged
template <class F>
__global__ void __launch_bounds__(64)
msm_reduce_groups_redo_kernel(const XYZZ<F>* __restrict__ bsum, uint32_t half, uint32_t m, uint32_t groups_per_win,
                              const uint32_t* __restrict__ redo_list, const uint32_t* __restrict__ redo_count,
                              XYZZ<F>* __restrict__ lsum, XYZZ<F>* __restrict__ rsum) {
    const uint32_t nredo = *redo_count;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < nredo; r += gridDim.x * blockDim.x) {
        const uint32_t gid = redo_list[r];
        uint32_t w = gid / groups_per_win, g = gid % groups_per_win;
        const XYZZ<F>* B = bsum + (uint64_t)w * half + (uint64_t)g * m;
        XYZZ<F> running = xyzz_inf<F>(), local = xyzz_inf<F>();
        for (int j = (int)m - 1; j >= 0; j--) {
            running = add(running, load_pod<XYZZ<F>>(&B[j]));
            local = add(local, running);
        }
        store_pod(&lsum[gid], local);
        store_pod(&rsum[gid], running);
    }
}

// part[((w*nbits + b)*chunks + ch)] = sum of rsum[w][g] over the groups g of chunk ch (chunk_len groups, a power of two)
// whose index has bit b set.  grid = (chunks, nbits, nsets), one wave per block.
template <class F>
__global__ void __launch_bounds__(64)
msm_bit_partial_kernel(const XYZZ<F>* __restrict__ rsum, const XYZZ<F>* __restrict__ lsum, uint32_t groups_per_win,
                       uint32_t chunk_len, int log_chunk, XYZZ<F>* __restrict__ part) {
    // blockIdx.y == nbits - 1 (the last row of the grid) is not a bit: it sums the chunk of lsum, so that one launch and one
    // final segment sum produce every quantity the host needs
    __shared__ LazyPt<F> sh[64];
    __shared__ XYZZ<F> shx[64];
    __shared__ uint32_t bad;
    const uint32_t ch = blockIdx.x, b = blockIdx.y, w = blockIdx.z;
    const uint32_t nbits = gridDim.y, chunks = gridDim.x;
    const uint32_t base = ch * chunk_len;
    const XYZZ<F>* R = rsum + (uint64_t)w * groups_per_win;
    XYZZ<F>* dst = &part[((uint64_t)w * nbits + b) * chunks + ch];
    if (b == nbits - 1) {
        const XYZZ<F>* Lp = lsum + (uint64_t)w * groups_per_win;
        block_sum29<F>(chunk_len, [&](uint32_t i) { return &Lp[base + i]; }, dst, sh, shx, &bad);
    } else if ((int)b >= log_chunk) {
        // the whole chunk has the bit set, or none of it
        block_sum29<F>(((base >> b) & 1) ? chunk_len : 0u, [&](uint32_t i) { return &R[base + i]; }, dst, sh, shx, &bad);
    } else {
        // insert a 1 at bit position b of the local index
        block_sum29<F>(chunk_len / 2, [&](uint32_t i) { return &R[base + (((i >> b) << (b + 1)) | (1u << b) | (i & ((1u << b) - 1)))]; }, dst, sh,
                       shx, &bad);
    }
}

// the same per-segment sum in the lazy representation (window reduction of large bucket sets)
template <class F>
__global__ void __launch_bounds__(64)
msm_segment_sum29_kernel(const XYZZ<F>* __restrict__ in, uint32_t seg_len, XYZZ<F>* __restrict__ out) {
    __shared__ LazyPt<F> sh[64];
    __shared__ XYZZ<F> shx[64];
    __shared__ uint32_t bad;
    const uint64_t base = (uint64_t)blockIdx.x * seg_len;
    block_sum29<F>(seg_len, [&](uint32_t i) { return &in[base + i]; }, &out[blockIdx.x], sh, shx, &bad);
}

// out[b] = sum of in[b*seg_len .. (b+1)*seg_len): one wave per segment, strided partial sums + LDS tree
template <class F>
__global__ void __launch_bounds__(64)
msm_segment_sum_kernel(const XYZZ<F>* __restrict__ in, uint32_t seg_len, XYZZ<F>* __restrict__ out) {
    __shared__ XYZZ<F> sh[64];
    const uint64_t base = (uint64_t)blockIdx.x * seg_len;
    XYZZ<F> acc = xyzz_inf<F>();
    for (uint32_t g = threadIdx.x; g < seg_len; g += 64) acc = add(acc, load_pod<XYZZ<F>>(&in[base + g]));
    acc = wave_tree_sum(acc, sh);
    if (threadIdx.x == 0) store_pod(&out[blockIdx.x], acc);
}

// ---- host: plan, merge, the two reductions, the combines -----------------------------------------------------------------------
// How the bucket sets of a call are reduced; computed once (no device work) and handed to the stages below.
struct MsmReducePlan {
    int nsets;                  // bucket sets: P.nsets, or the tables of a multi-table pass
    uint32_t m_groups;          // buckets per running-sum group
    uint32_t groups_per_win, total_groups;
    bool big_set, lazy;
};
inline MsmReducePlan msm_reduce_plan(Ctx* ctx, const void* d_bases, const MsmPrepared& P, int ntab) {
    MsmReducePlan R;
    const uint32_t half = P.half;
    R.nsets = ntab > 1 ? ntab : P.nsets;
    // buckets per running-sum group: MSM_GROUP when there are plenty of buckets, smaller (down to 2) when a set has few so
    // that the reduction still spreads over >= 2^15 lanes (small n, or table mode's single bucket set)
    const int tuned_group = ctx->tun.msm_group.load(std::memory_order_relaxed);
    R.m_groups = tuned_group ? (uint32_t)tuned_group : (uint32_t)MSM_GROUP;
    const uint64_t min_lanes = 32768;   // (65536 / 131072 measured in round 2: no change / slower)
    while (R.m_groups > 2 && (uint64_t)half * R.nsets / R.m_groups < min_lanes) R.m_groups >>= 1;
    if (R.m_groups > half) R.m_groups = half;
    R.groups_per_win = half / R.m_groups;
    R.total_groups = R.groups_per_win * R.nsets;
    // Large bucket sets: lazy per-group pass without the per-lane scalar multiplication,
    //   set sum = sum_g lsum[g] + m * sum_b 2^b * T_b,   T_b = sum of rsum[g] over the groups whose index has bit b set,
    // the T_b being plain tree sums and the last line host arithmetic.  Tiny sets keep the exact kernel: empty buckets (which
    // the lazy formulas cannot add to themselves) are the rule there and every group would be redone.
    // buckets from which the lazy pass pays (measured: 2^20 points / 2^16 buckets 2.82 -> 2.53 ms); ctx->tun is read from the
    // environment once per entry point (GA_REDUCE_LAZY_MIN: tests force the lazy path on sparse bucket sets with 0)
    // ... unless the set is DENSE (a table's shared set: windows x n entries over 2^(c-1) buckets; >= 16 entries per bucket leave
    // e^-16 of them empty): a 2^14-constraint proof spent 1.1 ms per MSM in the exact kernel's per-lane scalar multiplications
    // (6.3 ms per proof against 3.2 ms at 2^16, profiles/README.md round 3 batch N)
    // P.m counts every (scalar, window) pair, the zero digits in the skip bucket included: a table over which a 0/1-heavy witness
    // runs looks dense by that count while most of its buckets are empty.  The pair count of the skip bucket is only known on the
    // device at this point, so the verdict comes from the previous call on the same table: when the lazy pass flagged more than a
    // quarter of the groups, the set is remembered as sparse and small sets take the exact kernel again.
    R.big_set = (uint64_t)half * R.nsets >= ctx->tun.reduce_lazy_min;
    // (P.m and half describe ONE table's pairs and buckets; the tables of a multi-table pass share the scalar vector, hence the verdict)
    const bool dense_set = P.m >= 16ull * (uint64_t)half * (uint64_t)P.nsets && !(P.table && ctx->is_sparse_set(d_bases));
    R.lazy = R.big_set || dense_set;
    return R;
}

// Stage 5.  Scratch of the merge; its two counters ([0] hot buckets, [1] very hot buckets) are zeroed on the stream here, ahead of
// the bucket pass.
template <class F>
struct MsmMerge {
    uint32_t *hot_list, *hot_count, *vhot_list;
    XYZZ<F>* vtmp;
    uint32_t vtmp_stride;
};
template <class F>
int msm_merge_scratch(Ctx* ctx, const MsmPrepared& P, int ntab, hipStream_t st, MsmMerge<F>* M) {
    const uint64_t vhot_cap = P.max_tasks / MSM_VHOT_TASKS + 2;
    GA_CHECK(ctx->scratch_get("msm_hot", ((uint64_t)P.nb + 2) * 4, (void**)&M->hot_list));
    GA_CHECK(ctx->scratch_get("msm_hot_count", 256, (void**)&M->hot_count));
    GA_CHECK(ctx->scratch_get("msm_vhot", vhot_cap * 4, (void**)&M->vhot_list));
    GA_CHECK(ctx->scratch_get("msm_vhot_tmp", (uint64_t)ntab * vhot_cap * MSM_VHOT_SPLIT * sizeof(XYZZ<F>), (void**)&M->vtmp));
    M->vtmp_stride = (uint32_t)(vhot_cap * MSM_VHOT_SPLIT);
    GA_HIP_CHECK(hipMemsetAsync(M->hot_count, 0, 8, st));
    return GA_OK;
}
// sums = what the bucket pass wrote, [ntab x nb bucket sums | ntab x max_tasks partial sums]: on return every bucket sum is complete
template <class F>
int msm_merge(Ctx* ctx, const MsmPrepared& P, int ntab, hipStream_t st, const MsmMerge<F>& M, XYZZ<F>* sums) {
    StageTimer tm(ctx, "msm_merge");
    const uint32_t nb = P.nb, part_stride = (uint32_t)P.max_tasks;
    const unsigned ny = (unsigned)ntab;
    XYZZ<F>* bsum = sums;
    const XYZZ<F>* partial = sums + (uint64_t)ntab * nb;
    const uint32_t *task_off = P.task_off, *hot_count = M.hot_count, *vhot_count = M.hot_count + 1;
    hipLaunchKernelGGL((msm_merge_kernel<F>), dim3((nb + 255) / 256, ny), dim3(256), 0, st, partial, task_off, nb, bsum, M.hot_list, M.hot_count,
                       M.vhot_list, M.hot_count + 1, part_stride);
    hipLaunchKernelGGL((msm_hot_kernel<F>), dim3(512, ny), dim3(64), 0, st, partial, task_off, (const uint32_t*)M.hot_list, hot_count, bsum, nb,
                       part_stride);
    hipLaunchKernelGGL((msm_vhot_stage1_kernel<F>), dim3(2048, ny), dim3(64), 0, st, partial, task_off, (const uint32_t*)M.vhot_list, vhot_count,
                       M.vtmp, part_stride, M.vtmp_stride);
    hipLaunchKernelGGL((msm_vhot_stage2_kernel<F>), dim3(256, ny), dim3(64), 0, st, (const XYZZ<F>*)M.vtmp, (const uint32_t*)M.vhot_list,
                       vhot_count, bsum, nb, M.vtmp_stride);
    GA_KERNEL_CHECK();
    return GA_OK;
}

// Stage 6.  What a reduction leaves on the device for the host combine: `per_set` rows for each of the plan's sets.
template <class F>
struct MsmRows {
    const XYZZ<F>* d = nullptr;
    int per_set = 1;                           // exact: the set's sum.  lazy: rows 0..per_set-2 = the per-bit sums T_b of rsum, the last row = the sum of lsum
    const uint32_t* flagged_groups = nullptr;  // lazy: the device count of the groups that had to be redone exactly
};

// the exact reduction (tiny, sparse bucket sets): per-lane scalar multiplications, one sum per set
template <class F>
int msm_reduce_exact(Ctx* ctx, const MsmReducePlan& R, uint32_t half, const XYZZ<F>* bsum, hipStream_t st, MsmRows<F>* rows) {
    XYZZ<F>*gsum, *gsum2, *wsum;
    GA_CHECK(ctx->scratch_get("msm_gsum", (uint64_t)R.total_groups * sizeof(XYZZ<F>), (void**)&gsum));
    GA_CHECK(ctx->scratch_get("msm_gsum2", ((uint64_t)R.total_groups / 1024 + 64) * sizeof(XYZZ<F>), (void**)&gsum2));
    GA_CHECK(ctx->scratch_get("msm_wsum", (uint64_t)R.nsets * sizeof(XYZZ<F>), (void**)&wsum));
    StageTimer tm(ctx, "msm_reduce");
    hipLaunchKernelGGL((msm_reduce_groups_kernel<F>), dim3((R.total_groups + 63) / 64), dim3(64), 0, st, bsum, half, R.m_groups, R.groups_per_win,
                       R.total_groups, gsum);
    // set sum = sum of its group results; two levels when a set has many groups so that the first level spreads
    // over >= 16 waves per set instead of one
    const uint32_t sg = 1024;
    if (R.groups_per_win > 2 * sg) {
        const uint32_t nseg = R.groups_per_win / sg;   // powers of two: exact
        hipLaunchKernelGGL((msm_segment_sum_kernel<F>), dim3(nseg * R.nsets), dim3(64), 0, st, (const XYZZ<F>*)gsum, sg, gsum2);
        hipLaunchKernelGGL((msm_segment_sum_kernel<F>), dim3(R.nsets), dim3(64), 0, st, (const XYZZ<F>*)gsum2, nseg, wsum);
    } else {
        hipLaunchKernelGGL((msm_segment_sum_kernel<F>), dim3(R.nsets), dim3(64), 0, st, (const XYZZ<F>*)gsum, R.groups_per_win, wsum);
    }
    GA_KERNEL_CHECK();
    rows->d = wsum;
    return GA_OK;
}

// the lazy reduction: per-group running sums without the scalar multiplication, per-bit tree sums, the doublings left to the host
template <class F>
int msm_reduce_lazy(Ctx* ctx, const MsmReducePlan& R, uint32_t half, const XYZZ<F>* bsum, hipStream_t st, MsmRows<F>* rows) {
    const int nbits = ilog2_u64(R.groups_per_win), nsets = R.nsets;
    // chunk of groups per wave of the per-bit sums: 1024 where the grid fills the device anyway (2^24: 128 chunks x 18 rows; 256 / 128
    // measured there: msm_reduce 1.05 -> 1.13 / 1.34 ms, the second-level sums grow).  Smaller bucket sets are latency-bound -- a
    // lane's 16 dependent additions + 6 tree levels at ~9 us each made this kernel as expensive as the bucket accumulation of a
    // 2^16 MSM (profiles/README.md round 3, batches K / L) -- so the chunk shrinks until the grid has ~2 waves per SIMD
    uint32_t sg = 1024;
    while (sg > 64 && (uint64_t)(R.groups_per_win / sg) * (uint64_t)(nbits + 1) * (uint64_t)nsets < 2048) sg >>= 1;
    const uint32_t chunk_len = R.groups_per_win > sg ? sg : R.groups_per_win;   // powers of two
    const uint32_t chunks = R.groups_per_win / chunk_len;
    const int log_chunk = ilog2_u64(chunk_len);
    XYZZ<F>*gsum, *rsum, *bpart, *bits;
    uint32_t *rg_list, *rg_count;
    GA_CHECK(ctx->scratch_get("msm_gsum", (uint64_t)R.total_groups * sizeof(XYZZ<F>), (void**)&gsum));
    GA_CHECK(ctx->scratch_get("msm_rsum", (uint64_t)R.total_groups * sizeof(XYZZ<F>), (void**)&rsum));
    GA_CHECK(ctx->scratch_get("msm_bpart", ((uint64_t)nsets * (nbits + 1) * chunks + 64) * sizeof(XYZZ<F>), (void**)&bpart));
    GA_CHECK(ctx->scratch_get("msm_bits", ((uint64_t)nsets * (nbits + 1) + 64) * sizeof(XYZZ<F>), (void**)&bits));
    GA_CHECK(ctx->scratch_get("msm_redo_groups", ((uint64_t)R.total_groups + 2) * 4, (void**)&rg_list));
    GA_CHECK(ctx->scratch_get("msm_redo_groups_count", 256, (void**)&rg_count));
    GA_HIP_CHECK(hipMemsetAsync(rg_count, 0, 4, st));
    StageTimer tm(ctx, "msm_reduce");
    hipLaunchKernelGGL((msm_reduce_groups29_kernel<F>), dim3((R.total_groups + 63) / 64), dim3(64), 0, st, bsum, half, R.m_groups,
                       R.groups_per_win, R.total_groups, gsum, rsum, rg_list, rg_count);
    hipLaunchKernelGGL((msm_reduce_groups_redo_kernel<F>), dim3(256), dim3(64), 0, st, bsum, half, R.m_groups, R.groups_per_win,
                       (const uint32_t*)rg_list, (const uint32_t*)rg_count, gsum, rsum);
    // rows 0..nbits-1: per-bit sums of rsum; row nbits: sum of lsum
    hipLaunchKernelGGL((msm_bit_partial_kernel<F>), dim3(chunks, (unsigned)nbits + 1, (unsigned)nsets), dim3(64), 0, st,
                       (const XYZZ<F>*)rsum, (const XYZZ<F>*)gsum, R.groups_per_win, chunk_len, log_chunk, bpart);
    hipLaunchKernelGGL((msm_segment_sum29_kernel<F>), dim3((unsigned)(nsets * (nbits + 1))), dim3(64), 0, st, (const XYZZ<F>*)bpart,
                       chunks, bits);
    GA_KERNEL_CHECK();
    rows->d = bits;
    rows->per_set = nbits + 1;
    rows->flagged_groups = rg_count;
    return GA_OK;
}

// ---- the host combines: the last doublings of a call, sequential and latency-bound on a GPU lane, free on a host core ----------
// exact reduction, un-pinned bases: Horner over the window sums ws[0, nsets), sum_w 2^(c w) ws[w]
template <class F>
XYZZ<F> msm_combine_horner(const XYZZ<F>* ws, int nsets, int c) {
    XYZZ<F> acc = xyzz_inf<F>();
    for (int w = nsets - 1; w >= 0; w--) {
        for (int k = 0; k < c; k++) acc = dbl(acc);
        acc = add(acc, ws[w]);
    }
    return acc;
}
// lazy reduction, one set's rows hb[0, nbits]: L + 2^log_m * sum_b 2^b T_b -- ~nbits + log2(m) doublings and nbits additions
template <class F>
XYZZ<F> msm_combine_set(const XYZZ<F>* hb, int nbits, int log_m) {
    XYZZ<F> acc = xyzz_inf<F>();
    for (int b = nbits - 1; b >= 0; b--) acc = add(dbl(acc), hb[b]);
    for (int k = 0; k < log_m; k++) acc = dbl(acc);
    return add(hb[nbits], acc);
}
// lazy reduction, un-pinned bases: result = sum_w 2^(c w) [ L_w + 2^log_m * sum_b 2^b T_(w,b) ]: every term has a bit position (c w
// for L_w, c w + log_m + b for T_(w,b)), and ONE descent over the positions -- a doubling per position, an addition per term --
// replaces the per-set chains (nbits + log_m doublings each) followed by the Horner step over the windows (c doublings each):
// 255 + 16 doublings instead of 15 x 16 + 255 for a 2^20-point MSM (c = 17), 0.1 ms of the 0.35 ms the host spent per call.
template <class F>
XYZZ<F> msm_combine_descent(const XYZZ<F>* hb, int nsets, int nbits, int log_m, int c) {
    const int rows = nbits + 1, top = c * (nsets - 1) + log_m + nbits - 1;
    std::vector<std::vector<const XYZZ<F>*>> at((size_t)top + 1);
    for (int w = 0; w < nsets; w++) {
        at[(size_t)(c * w)].push_back(&hb[(size_t)w * rows + nbits]);
        for (int b = 0; b < nbits; b++) at[(size_t)(c * w + log_m + b)].push_back(&hb[(size_t)w * rows + b]);
    }
    XYZZ<F> acc = xyzz_inf<F>();
    for (int pos = top; pos >= 0; pos--) {
        if (pos != top) acc = dbl(acc);
        for (const XYZZ<F>* t : at[(size_t)pos]) acc = add(acc, *t);
    }
    return acc;
}
// the rows of a reduction (host copies) -> the results of the call: one per set, or (horner_c > 0) their combination in out[0]
template <class F>
void msm_combine(const MsmReducePlan& R, const XYZZ<F>* h, int per_set, int horner_c, XYZZ<F>* out) {
    const int nbits = per_set - 1, log_m = ilog2_u64(R.m_groups);
    if (!R.lazy) {
        if (horner_c > 0) out[0] = msm_combine_horner(h, R.nsets, horner_c);
        else
            for (int w = 0; w < R.nsets; w++) out[w] = h[w];
    } else if (horner_c > 0) {
        out[0] = msm_combine_descent(h, R.nsets, nbits, log_m, horner_c);
    } else {
        for (int w = 0; w < R.nsets; w++) out[w] = msm_combine_set(h + (size_t)w * per_set, nbits, log_m);
    }
}

}  // namespace ga

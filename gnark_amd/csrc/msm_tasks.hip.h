// Stage 3 of the MSM pipeline (msm.hip.h): sorted pairs -> bucket boundaries -> the length-ordered task list; and msm_prepare, the
// group-independent half of an MSM as plan -> sort -> tasks.
#pragma once
#include "msm_sort.hip.h"

namespace ga {

// The task list is sorted on at most 8 key bits below 2^25 pairs (msm_build_tasks): ONE onesweep pass.  The library's default switches
// to a merge sort below 2^20 items -- 20 launches, 0.14 ms, for the 1.04 M tasks of a 2^20-point MSM
// (profiles/r05_h_msm_2p20_raw_kernels_seg256.txt) -- so the limit is lowered to where a merge sort is really cheaper.
typedef rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, 32768> MsmTaskSort;

// ---- 3. bucket boundaries and tasks ---------------------------------------------------------------
// bucket boundaries by binary search + the number of tasks per bucket, one launch (library-sort path: small MSMs, where every launch
// is ~5 us of a ~2 ms call): a block shares its boundaries in LDS
static __global__ void __launch_bounds__(256) msm_offsets_tasks_kernel(const uint32_t* __restrict__ keys, uint64_t m, uint32_t nb, uint32_t seg,
                                                                       uint32_t* __restrict__ off, uint32_t* __restrict__ ntask) {
    __shared__ uint32_t sh[257];
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    auto lower = [&](uint32_t key) {   // first index with keys[idx] >= key
        uint64_t lo = 0, hi = m;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (keys[mid] < key) lo = mid + 1;
            else hi = mid;
        }
        return (uint32_t)lo;
    };
    if (b <= nb) {
        sh[threadIdx.x] = lower(b);
        off[b] = sh[threadIdx.x];
        if (threadIdx.x == blockDim.x - 1 && b < nb) sh[blockDim.x] = lower(b + 1);
    }
    __syncthreads();
    if (b <= nb) ntask[b] = b < nb ? (sh[threadIdx.x + 1] - sh[threadIdx.x] + seg - 1) / seg : 0;
}

static __global__ void msm_tasks_kernel(const uint32_t* __restrict__ off, uint32_t nb, uint32_t seg, uint32_t* __restrict__ ntask) {
    uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b > nb) return;
    uint32_t sz = b < nb ? off[b + 1] - off[b] : 0;
    ntask[b] = (sz + seg - 1) / seg;
}

// task t of bucket b covers sorted pairs [start, start+len); key = SEG - len so that an ascending radix sort puts the
// longest tasks first and lanes of one wave get tasks of (nearly) equal length (bucket sizes are Poisson-distributed:
// without this a wave waits for its longest bucket, ~25 % of the lanes' time at 2^24).  Below 2^25 pairs the SORT key is the length
// quantised to 7 bits (qkey = key >> qshift; lanes of a wave then differ by < 2^qshift points): with the padding bit that is ONE
// 8-bit radix pass over the task list instead of two (2^20 raw MSM: task stage 0.18 -> 0.08 ms, profiles/r05_e); the exact key
// stays in task_key.  From 2^25 pairs up the sort key IS the exact key: the second pass costs ~0.02 ms, lanes that wait for a
// neighbour 1-3 points longer cost the bucket kernel 1.4 % (15.40 -> 15.62 ms at 12 x 2^24 pairs, same box against round 4's
// exact sort, profiles/r05_w_round4_vs_round5_same_box.txt).
// (one launch for what were two memsets and an iota: padding keys, the identity permutation the task sort starts from, the counter
// of the long-bucket queue)
static __global__ void msm_task_init_kernel(uint32_t* __restrict__ task_qkey, uint32_t* __restrict__ task_id, uint32_t n, uint32_t* __restrict__ long_count) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        task_qkey[i] = 0xFFFFFFFFu;
        task_id[i] = i;
    }
    if (i == 0) *long_count = 0;
}

// Buckets with more than MSM_LONG_TASKS tasks (a boolean-heavy witness puts millions of points into the digit-1 bucket of window 0)
// are not written by their one lane: they are queued and written by msm_task_list_long_kernel, a block per bucket.
constexpr uint32_t MSM_LONG_TASKS = 64;
static __global__ void msm_task_list_kernel(const uint32_t* __restrict__ off, const uint32_t* __restrict__ task_off, uint32_t nb,
                                            uint32_t seg, int qshift, uint32_t* __restrict__ task_start, uint32_t* __restrict__ task_key,
                                            uint32_t* __restrict__ task_qkey, uint32_t* __restrict__ task_dest, uint32_t* __restrict__ long_list,
                                            uint32_t* __restrict__ long_count) {
    uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    uint32_t t0 = task_off[b], t1 = task_off[b + 1];
    uint32_t start = off[b], end = off[b + 1];
    if (t1 - t0 > MSM_LONG_TASKS) {
        long_list[atomicAdd(long_count, 1u)] = b;
        return;
    }
    for (uint32_t t = t0; t < t1; t++) {
        uint32_t len = end - start < seg ? end - start : seg;
        task_start[t] = start;
        // where the task's sum goes in the array [nb bucket sums | partial sums]: the only task of a bucket writes the bucket
        // sum itself (the merge pass then has nothing to do for that bucket)
        task_dest[t] = (t1 - t0 == 1) ? b : nb + t;
        task_key[t] = seg - len;
        task_qkey[t] = (seg - len) >> qshift;
        start += len;
    }
}

static __global__ void msm_task_list_long_kernel(const uint32_t* __restrict__ off, const uint32_t* __restrict__ task_off, uint32_t nb, uint32_t seg,
                                                 int qshift, uint32_t* __restrict__ task_start, uint32_t* __restrict__ task_key,
                                                 uint32_t* __restrict__ task_qkey, uint32_t* __restrict__ task_dest,
                                                 const uint32_t* __restrict__ long_list, const uint32_t* __restrict__ long_count) {
    const uint32_t nl = *long_count;
    for (uint32_t h = blockIdx.x; h < nl; h += gridDim.x) {
        const uint32_t b = long_list[h];
        const uint32_t t0 = task_off[b], t1 = task_off[b + 1];
        const uint32_t start = off[b], end = off[b + 1];
        for (uint32_t t = t0 + threadIdx.x; t < t1; t += blockDim.x) {   // every task but the last is full
            const uint32_t s0 = start + (t - t0) * seg;
            const uint32_t len = end - s0 < seg ? end - s0 : seg;
            task_start[t] = s0;
            task_dest[t] = nb + t;
            task_key[t] = seg - len;
            task_qkey[t] = (seg - len) >> qshift;
        }
    }
}

// ---- host: plan -> sort -> tasks ---------------------------------------------------------------------------------------------
// The arithmetic of a call, no device work: checks the arguments and fills the scalar fields of *P (untouched on error).  bits: of
// the scalar field.  end_bit: the significant key bits of the library sort.
inline int msm_plan_prepare(Ctx* ctx, int bits, size_t n, int c, int win_lo, int win_hi, bool table, int batch, MsmPrepared* P, int* end_bit) {
    const int nwin = bits / c + 1;
    if (win_hi < 0) win_hi = nwin;
    if (win_lo < 0 || win_hi > nwin || win_lo >= win_hi || c < 2 || c > 24) {
        set_error("msm: bad window range [%d,%d) of %d (c=%d, table=%d)", win_lo, win_hi, nwin, c, (int)table);
        return GA_ERR_INVALID;
    }
    const int nwl = win_hi - win_lo;
    if (n == 0 || n >= (1ull << 31)) {
        set_error("msm: n=%zu outside [1, 2^31)", n);
        return GA_ERR_INVALID;
    }
    if (batch < 1 || (batch > 1 && !table)) {
        set_error("msm: a batch of scalar vectors needs a precomputed table (batch=%d, table=%d)", batch, (int)table);
        return GA_ERR_INVALID;
    }
    const uint32_t half = 1u << (c - 1);
    const uint64_t m = (uint64_t)batch * nwl * n;
    const uint64_t nb = table ? (uint64_t)batch * half : (uint64_t)nwl * half;
    // table mode: the value indexes the WHOLE table [window][point] even when only a window range is accumulated (multi-GPU
    // partition A on pinned bases: the 2^(c*w) factors are baked into the table, so partial results simply add)
    if (m >= (1ull << 31) || nb >= (1ull << 31) || (table && (uint64_t)nwin * n >= (1ull << 31))) {
        set_error("msm: %d windows x %zu points exceeds the 2^31 pair index space; shard the call", nwl, n);
        return GA_ERR_INVALID;
    }
    // task length: buckets up to 4x the mean size stay one task, unless that would leave fewer than ~2^20 tasks for the
    // 256 CUs x 16 waves x 64 lanes (few-bucket cases: small n, or table mode where all windows share 2^(c-1) buckets)
    const uint64_t mean = m / nb + 1;
    const uint64_t min_seg = ctx->tun.msm_min_seg;
    uint64_t seg = mean * 4 < min_seg ? min_seg : mean * 4;
    if (nb < (1u << 19)) {
        uint64_t want = (m >> 19) + 1, lo = mean / 6 > 32 ? mean / 6 : 32;   // keep a bucket's partials <= ~MSM_HOT_TASKS (msm_reduce.hip.h)
        if (want < lo) want = lo;
        if (want < seg) seg = want;
    }
    *end_bit = 1;
    while ((1ull << *end_bit) <= nb) (*end_bit)++;   // keys take values 0..nb (nb = SKIP)
    P->n = n;
    P->c = c;
    P->nwin = nwin;
    P->win_lo = win_lo;
    P->win_hi = win_hi;
    P->nsets = table ? batch : nwl;
    P->table = table;
    P->half = half;
    P->nb = (uint32_t)nb;
    P->seg = (uint32_t)seg;
    P->m = m;
    P->max_tasks = nb + m / P->seg + 1;
    return GA_OK;
}

// Stage 3 on the stream: the explicit task list of the sorted pairs, ordered by decreasing length (padding slots keep key =
// 0xFFFFFFFF >= seg); fills the task arrays of *P.  off / sorted_keys: what msm_sort returned.
inline int msm_build_tasks(Ctx* ctx, const std::string& sfx, hipStream_t st, uint32_t* off, const uint32_t* sorted_keys, MsmPrepared* P) {
    auto key = [&](const char* k) { return std::string(k) + sfx; };
    const uint32_t nb = P->nb, seg = P->seg;
    const uint64_t max_tasks = P->max_tasks;
    uint32_t *ntask, *task_off, *task_start, *task_key, *task_key2, *task_qkey, *task_id, *task_perm, *task_dest, *long_list, *long_count;
    void* tmp;
    GA_CHECK(ctx->scratch_get(key("msm_ntask").c_str(), ((uint64_t)nb + 2) * 4, (void**)&ntask));
    GA_CHECK(ctx->scratch_get(key("msm_task_off").c_str(), ((uint64_t)nb + 2) * 4, (void**)&task_off));
    GA_CHECK(ctx->scratch_get(key("msm_task_start").c_str(), max_tasks * 4, (void**)&task_start));
    GA_CHECK(ctx->scratch_get(key("msm_task_key").c_str(), max_tasks * 4, (void**)&task_key));
    GA_CHECK(ctx->scratch_get(key("msm_task_key2").c_str(), max_tasks * 4, (void**)&task_key2));
    GA_CHECK(ctx->scratch_get(key("msm_task_qkey").c_str(), max_tasks * 4, (void**)&task_qkey));
    GA_CHECK(ctx->scratch_get(key("msm_task_id").c_str(), max_tasks * 4, (void**)&task_id));
    GA_CHECK(ctx->scratch_get(key("msm_task_perm").c_str(), max_tasks * 4, (void**)&task_perm));
    GA_CHECK(ctx->scratch_get(key("msm_task_dest").c_str(), max_tasks * 4, (void**)&task_dest));
    StageTimer tm(ctx, "msm_tasks", st);
    GA_CHECK(ctx->scratch_get(key("msm_long").c_str(), (max_tasks / MSM_LONG_TASKS + 2) * 4, (void**)&long_list));
    GA_CHECK(ctx->scratch_get(key("msm_long_count").c_str(), 256, (void**)&long_count));
    int kbits = 1;
    while ((1u << kbits) <= seg) kbits++;
    // (long lists: the exact length, two radix passes -- GA_MSM_TASK_EXACT_MIN, see msm_task_init_kernel)
    const bool exact = P->m >= ctx->tun.msm_task_exact_min.load(std::memory_order_relaxed);
    const int qbits = exact || kbits < 7 ? kbits : 7, qshift = kbits - qbits;
    hipLaunchKernelGGL(msm_task_init_kernel, dim3((unsigned)((max_tasks + 255) / 256)), dim3(256), 0, st, task_qkey, task_id, (uint32_t)max_tasks, long_count);
    if (sorted_keys)
        hipLaunchKernelGGL(msm_offsets_tasks_kernel, dim3((nb + 1 + 255) / 256), dim3(256), 0, st, sorted_keys, P->m, nb, seg, off, ntask);
    else   // (the fused sort produced `off` itself)
        hipLaunchKernelGGL(msm_tasks_kernel, dim3((nb + 1 + 255) / 256), dim3(256), 0, st, (const uint32_t*)off, nb, seg, ntask);
    GA_KERNEL_CHECK();
    size_t tmp_bytes = 0;
    GA_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, ntask, task_off, (int)(nb + 1), st));
    GA_CHECK(ctx->scratch_get(key("msm_scan_tmp").c_str(), tmp_bytes + 256, &tmp));
    GA_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, ntask, task_off, (int)(nb + 1), st));
    hipLaunchKernelGGL(msm_task_list_kernel, dim3((nb + 255) / 256), dim3(256), 0, st, (const uint32_t*)off, (const uint32_t*)task_off,
                       nb, seg, qshift, task_start, task_key, task_qkey, task_dest, long_list, long_count);
    hipLaunchKernelGGL(msm_task_list_long_kernel, dim3(256), dim3(256), 0, st, (const uint32_t*)off, (const uint32_t*)task_off, nb, seg,
                       qshift, task_start, task_key, task_qkey, task_dest, (const uint32_t*)long_list, (const uint32_t*)long_count);
    GA_KERNEL_CHECK();
    // padding keys are all-ones: sort on qbits+1 bits so that they stay behind every real key (real keys < 2^qbits)
    size_t tb = 0;
    GA_HIP_CHECK((rocprim::radix_sort_pairs<MsmTaskSort>(nullptr, tb, task_qkey, task_key2, task_id, task_perm, (size_t)max_tasks, 0u, (unsigned)(qbits + 1), st)));
    GA_CHECK(ctx->scratch_get(key("msm_tasksort_tmp").c_str(), tb + 256, &tmp));
    GA_HIP_CHECK((rocprim::radix_sort_pairs<MsmTaskSort>(tmp, tb, task_qkey, task_key2, task_id, task_perm, (size_t)max_tasks, 0u, (unsigned)(qbits + 1), st)));
    P->task_off = task_off;
    P->task_start = task_start;
    P->task_key = task_key2;
    P->task_key_by_id = task_key;
    P->task_perm = task_perm;
    P->task_dest = task_dest;
    return GA_OK;
}

// The group-independent half of an MSM.  batch > 1 (table mode only): `d_scalars` is an array of `batch` device pointers, one scalar
// vector each, over the SAME table: one sort, one task list, one bucket set per vector (P->nsets = batch) -- the three wire
// commitments or the three quotient shards of a PLONK proof share every launch and every latency-bound tail.
template <class FrP>
int msm_prepare(Ctx* ctx, const void* d_scalars, size_t n, bool scalars_mont, int c, int win_lo, int win_hi, bool table,
                MsmPrepared* P, int slot = 0, int batch = 1) {
    hipStream_t st = ctx->work_stream();
    const std::string sfx = slot ? "#1" : "";
    int end_bit;
    GA_CHECK(msm_plan_prepare(ctx, FrP::BITS, n, c, win_lo, win_hi, table, batch, P, &end_bit));
    const MsmScalars S{d_scalars, n, scalars_mont, batch};
    uint32_t* off;
    const uint32_t* sorted_keys;
    GA_CHECK((msm_sort<FrP>(ctx, sfx, st, S, end_bit, P, &off, &sorted_keys)));
    return msm_build_tasks(ctx, sfx, st, off, sorted_keys, P);
}

}  // namespace ga

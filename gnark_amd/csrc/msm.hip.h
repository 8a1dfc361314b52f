// Pippenger multi-scalar multiplication for G1/G2 of BN254 and BLS12-381 on gfx950.
//
// Replaces G1Jac.MultiExp / G2Jac.MultiExp (backend/groth16/bn254/prove.go:194,207,227,237,283) and the ICICLE
// msm.Msm / g2.G2Msm calls (backend/accelerated/icicle/groth16/bn254/icicle.go:362-467).
//
// Pipeline (all on the context's stream, no host synchronisation until a few hundred bytes of sums are copied back), one header per
// stage; each stage is a host function that owns its scratch, and the two drivers -- msm_prepare (msm_tasks.hip.h) for the
// group-independent stages 1-3, msm_accumulate_reduce (below) for 4-6 -- are sequences of those calls:
//
// msm_sort.hip.h     (msm_sort)
//   1. msm_digits_kernel   scalar -> signed c-bit digits (Montgomery reduction fused in); one (key, value) pair per
//                          (point, window): key = window*2^(c-1) + |digit|-1, value = point index | sign<<31.
//                          Zero digits get key = SKIP (sorts last), so zero scalars and the constant-0 wires of a
//                          witness cost nothing downstream.
//   2. radix sort          of the pairs by key (rocprim onesweep on the significant bits only, msm_sort_pairs); after it every
//                          bucket is a contiguous run of point indices.
//      From GA_MSM_FUSE_MIN (2^21) pairs up, 1 and 2 are ONE two-level sort of our own, fused with the digit extraction
//      (1b / 1c, msm_fused_sort): the pairs are written once and read once, the sorted keys are never materialised.
// msm_tasks.hip.h    (msm_build_tasks; msm_plan_prepare, msm_prepare)
//   3. msm_offsets_tasks_kernel / msm_tasks_kernel  bucket boundaries (by binary search, or the fused sort's own per-key scan);
//                          buckets are split into tasks of at most SEG points so that a hot bucket (witness values 0/1 make
//                          bucket 1 of window 0 huge) is spread over many lanes; the task list is ordered by decreasing length
//                          (a radix sort on the length quantised to at most 7 bits plus the padding bit -- one 8-bit pass -- or,
//                          from GA_MSM_TASK_EXACT_MIN (2^25) pairs up, on the exact length) so that the lanes of a wave finish
//                          together.
// msm_bucket.hip.h   (msm_bucket_pass; the window-table build's kernel)
//   4. msm_accumulate29_kernel  one lane per task: gathers its bases from the window table (or the hat-domain copy of un-pinned
//                          bases), XYZZ mixed additions in the lazy 29 / 28-bit limb representation, accumulator in LDS.  Tasks
//                          in which an exceptional addition occurred are redone (complete lazy loop, then exact arithmetic).
// msm_reduce.hip.h   (msm_reduce_plan, msm_merge, msm_reduce_exact / msm_reduce_lazy, msm_combine)
//   5. msm_merge_kernel / msm_hot_kernel / msm_vhot_stage{1,2}_kernel  partial sums -> one XYZZ sum per bucket (wave-level LDS
//                          tree for hot buckets, two stages for very hot ones).
//   6. msm_reduce_groups29_kernel + per-bit / segment sums  sum_k k*B_k per bucket set via per-group running sums and a wave
//                          tree (tiny sparse sets: msm_reduce_groups_kernel, exact, with the per-lane scalar multiplication);
//                          the last ~c doublings of that sum -- and, for un-pinned bases, the Horner step over the windows,
//                          merged into the same chain -- run on the host: a chain of sequential doublings is latency-bound on a
//                          GPU lane and free on a host core, and the multi-GPU window-sharded mode needs the window sums on the
//                          host anyway.
// msm_lazy.hip.h     the general-point arithmetic in the lazy representation that 5, 6 and the table build share.
//
// This header: msm_accumulate_reduce, the per-(curve, group) launch sequences and -- at the end -- the drivers of the MSM calls of the C
// ABI (msm_run, msm_abi_run, msm_table_create_run, msm_table_run), all instantiated by the msm_<curve>_<group>.hip units.
#pragma once
#include "hostops.hip.h"
#include "vec_call.hip.h"
#include "msm_sort.hip.h"
#include "msm_tasks.hip.h"
#include "msm_bucket.hip.h"
#include "msm_reduce.hip.h"

namespace ga {

// Group-dependent half: bucket accumulation over `d_bases` (the affine bases, or the precomputed table in table mode),
// merge, per-set reduction.  Writes P.nsets XYZZ sums to host memory.
//
// horner_c > 0 (raw bases, every window of the call): instead of the P.nsets window sums, out[0] receives their combination
// sum_w 2^(horner_c * w) * set_w -- the window reduction's per-bit sums and the Horner step over the windows then share ONE chain of
// doublings on the host (msm_combine_descent).
//
// ntab > 1 (table mode, ONE scalar vector, `tables` = ntab tables of the same shape as d_bases -- the wire-indexed A, B1, K of a Groth16
// key): every kernel of the pipeline runs ONCE over all the tables -- the bucket kernel with the table as the grid's y dimension, the
// merge the same way, the window reduction over ntab bucket sets as it does for a batch of scalar vectors -- and out[i] receives
// table i's sum: one tail per kernel, one host synchronisation, ntab x the waves in the latency-bound reduction kernels.
template <class F>
int msm_accumulate_reduce(Ctx* ctx, const void* d_bases, const MsmPrepared& P, XYZZ<F>* out, int horner_c = 0, const void* const* tables = nullptr,
                          int ntab = 1) {
    if (ntab < 1 || ntab > 4 || (ntab > 1 && (!tables || !P.table || P.nsets != 1 || horner_c != 0))) {
        set_error("msm: a multi-table pass takes 2..4 precomputed tables over one prepared scalar vector (ntab=%d, table=%d, sets=%d)", ntab, (int)P.table, P.nsets);
        return GA_ERR_INVALID;
    }
    hipStream_t st = ctx->work_stream();
    const MsmReducePlan R = msm_reduce_plan(ctx, d_bases, P, ntab);
    MsmMerge<F> M;
    GA_CHECK(msm_merge_scratch(ctx, P, ntab, st, &M));
    PendingRead flags(ctx);   // from here on every return, an error's included, waits for the bucket pass's flag counts to have landed
    XYZZ<F>* sums;            // [bucket sums | partial sums]; the bucket sums are complete after the merge
    GA_CHECK(msm_bucket_pass<F>(ctx, d_bases, P, tables, ntab, st, flags, &sums));
    GA_CHECK(msm_merge<F>(ctx, P, ntab, st, M, sums));
    MsmRows<F> rows;
    if (R.lazy) GA_CHECK(msm_reduce_lazy<F>(ctx, R, P.half, sums, st, &rows));
    else GA_CHECK(msm_reduce_exact<F>(ctx, R, P.half, sums, st, &rows));
    // the one copy and the one synchronisation of a call: a few hundred bytes of sums (and the lazy reduction's count of flagged groups)
    std::vector<XYZZ<F>> h((size_t)R.nsets * rows.per_set);
    uint32_t flagged_groups = 0;
    GA_HIP_CHECK(hipMemcpyAsync(h.data(), rows.d, h.size() * sizeof(XYZZ<F>), hipMemcpyDeviceToHost, st));
    if (rows.flagged_groups) GA_HIP_CHECK(hipMemcpyAsync(&flagged_groups, rows.flagged_groups, 4, hipMemcpyDeviceToHost, st));
    GA_HIP_CHECK(hipStreamSynchronize(st));
    msm_note_degenerate(ctx, P, d_bases, tables, ntab, flags);
    if (R.lazy && P.table && !R.big_set) ctx->note_sparse_set(d_bases, (uint64_t)flagged_groups * 4 > R.total_groups);
    msm_combine(R, h.data(), rows.per_set, horner_c, out);
    return GA_OK;
}

template <class C, int G>
int msm_windows_device(Ctx* ctx, const void* d_bases, const void* d_scalars, size_t n, bool scalars_mont, int c,
                       int win_lo, int win_hi, void* h_window_sums, bool combine) {
    typedef typename GroupField<C, G>::F F;
    XYZZ<F>* out = reinterpret_cast<XYZZ<F>*>(h_window_sums);
    const int nwin = C::FrP::BITS / c + 1;
    if (win_hi < 0) win_hi = nwin;
    if (n == 0) {
        for (int w = 0; w < (combine ? 1 : win_hi - win_lo); w++) out[w] = xyzz_inf<F>();
        return GA_OK;
    }
    MsmPrepared P;
    GA_CHECK(msm_prepare<typename C::FrP>(ctx, d_scalars, n, scalars_mont, c, win_lo, win_hi, false, &P));
    // combine: out[0] = sum_w 2^(c (w - win_lo)) W_w; a window share that does not start at window 0 is shifted by the caller
    return msm_accumulate_reduce<F>(ctx, d_bases, P, out, combine ? c : 0);
}

// MSM over a precomputed table: one XYZZ result (no Horner); windows [win_lo, win_hi) only (win_hi < 0 = all): the partial
// sums of disjoint window ranges add up to the full result
template <class C, int G>
int msm_table_device(Ctx* ctx, const void* d_table, const void* d_scalars, size_t n, bool scalars_mont, int c, void* h_sum, int win_lo,
                     int win_hi) {
    typedef typename GroupField<C, G>::F F;
    XYZZ<F>* out = reinterpret_cast<XYZZ<F>*>(h_sum);
    if (n == 0 || (win_hi >= 0 && win_hi <= win_lo)) {
        *out = xyzz_inf<F>();
        return GA_OK;
    }
    MsmPrepared P;
    GA_CHECK(msm_prepare<typename C::FrP>(ctx, d_scalars, n, scalars_mont, c, win_lo, win_hi, true, &P));
    return msm_accumulate_reduce<F>(ctx, d_table, P, out);
}

// `batch` scalar vectors (host array of device pointers) over one table: batch XYZZ results
template <class C, int G>
int msm_table_device_batch(Ctx* ctx, const void* d_table, const void* const* d_scalars, int batch, size_t n, bool scalars_mont, int c,
                           void* h_sums) {
    typedef typename GroupField<C, G>::F F;
    XYZZ<F>* out = reinterpret_cast<XYZZ<F>*>(h_sums);
    if (n == 0) {
        for (int b = 0; b < batch; b++) out[b] = xyzz_inf<F>();
        return GA_OK;
    }
    MsmPrepared P;
    // (msm_prepare takes the vector itself for batch == 1, the pointer array otherwise)
    GA_CHECK(msm_prepare<typename C::FrP>(ctx, batch == 1 ? d_scalars[0] : (const void*)d_scalars, n, scalars_mont, c, 0, -1, true, &P, 0, batch));
    return msm_accumulate_reduce<F>(ctx, d_table, P, out);
}

// prepared scalars (table mode) reused for another base table of the same length (G1.B / G2.B)
template <class C, int G>
int msm_table_device_reuse(Ctx* ctx, const void* d_table, const MsmPrepared& P, void* h_sum) {
    typedef typename GroupField<C, G>::F F;
    return msm_accumulate_reduce<F>(ctx, d_table, P, reinterpret_cast<XYZZ<F>*>(h_sum));
}

// ... and for SEVERAL tables of that shape in one pass (the wire-indexed G1.A, G1.B, G1.K of a Groth16 key over the one witness sort,
// prove.go:194,207,237): h_sums[i] = the MSM over tables[i].  2 <= ntab <= 4.
template <class C, int G>
int msm_table_device_reuse_multi(Ctx* ctx, const void* const* tables, int ntab, const MsmPrepared& P, void* h_sums) {
    typedef typename GroupField<C, G>::F F;
    return msm_accumulate_reduce<F>(ctx, tables[0], P, reinterpret_cast<XYZZ<F>*>(h_sums), 0, tables, ntab);
}

// group-independent preparation callable from translation units that do not include this header (groth16.hip)
template <class C>
int msm_prepare_table_scalars(Ctx* ctx, const void* d_scalars, size_t n, bool scalars_mont, int c, MsmPrepared* P, int slot, int win_lo,
                              int win_hi, int batch) {
    return msm_prepare<typename C::FrP>(ctx, d_scalars, n, scalars_mont, c, win_lo, win_hi, true, P, slot, batch);
}

template <class C, int G>
size_t msm_table_point_bytes() {
    typedef typename GroupField<C, G>::F F;
    return Table29<F>::WORDS * 4;
}

template <class C, int G>
int msm_table_build(Ctx* ctx, const void* d_bases, size_t n, int c, void* d_table) {
    typedef typename GroupField<C, G>::F F;
    if (n == 0) return GA_OK;
    const int nwin = C::FrP::BITS / c + 1;
    StageTimer tm(ctx, "msm_table_build");
    hipLaunchKernelGGL((msm_table29_kernel<F>), dim3((unsigned)(((n + TableBatch<F>::K - 1) / TableBatch<F>::K + 63) / 64)), dim3(64), 0, ctx->work_stream(),
                       (const Affine<F>*)d_bases, (uint64_t)n, c, nwin, (uint32_t*)d_table);
    GA_KERNEL_CHECK();
    return GA_OK;
}

// ---- the drivers (declared in common.hip.h) -----------------------------------------------------------------------------------------
template <class C, int G>
int msm_run(Ctx* ctx, const void* d_bases, const void* d_scalars, size_t n, bool scalars_mont, int c, int win_lo, int win_hi, size_t max_chunk,
            void* h_out, bool want_windows) {
    typedef typename GroupField<C, G>::F F;
    XYZZ<F>* out = reinterpret_cast<XYZZ<F>*>(h_out);
    const size_t nw = (size_t)(win_hi - win_lo), pair_cap = ((size_t)1 << 31) / nw - 1;   // (never reached up to 2^26 points)
    if (max_chunk == 0 || max_chunk > pair_cap) max_chunk = pair_cap;
    XYZZ<F> sum;
    if (!want_windows && n <= max_chunk) {   // the usual case: one launch sequence, the Horner step shares the window reduction's host chain
        GA_CHECK((msm_windows_device<C, G>(ctx, d_bases, d_scalars, n, scalars_mont, c, win_lo, win_hi, &sum, true)));
    } else {
        std::vector<XYZZ<F>> W(nw, xyzz_inf<F>()), part(nw);
        for (size_t done = 0; done < n;) {
            const size_t cn = n - done < max_chunk ? n - done : max_chunk;
            GA_CHECK((msm_windows_device<C, G>(ctx, (const char*)d_bases + done * sizeof(Affine<F>), (const char*)d_scalars + done * 32, cn,
                                              scalars_mont, c, win_lo, win_hi, part.data())));
            for (size_t w = 0; w < nw; w++) W[w] = add(W[w], part[w]);
            done += cn;
        }
        if (want_windows) {
            for (size_t w = 0; w < nw; w++) out[w] = W[w];
            return GA_OK;
        }
        sum = host_horner(W.data(), (int)nw, c);
    }
    for (int k = 0; k < c * win_lo; k++) sum = dbl(sum);   // the windows below the range count as zero
    *out = sum;
    return GA_OK;
}

template <class C, int G>
int msm_abi_run(Ctx* ctx, const void* bases, const void* scalars, size_t n, unsigned flags, int win_lo, int win_hi, void* out, int* c_out,
                int* nwin_out, bool want_windows) {
    typedef typename GroupField<C, G>::F F;
    int c, nwin;
    GA_CHECK(msm_plan<C>(G, n, &c, &nwin));
    if (c_out) *c_out = c;
    if (nwin_out) *nwin_out = nwin;
    if (win_hi < 0) win_hi = nwin;
    if (win_lo < 0 || win_hi > nwin || win_lo >= win_hi) {
        set_error("msm: window range [%d,%d) outside [0,%d)", win_lo, win_hi, nwin);
        return GA_ERR_INVALID;
    }
    Staged sb{ctx}, ss{ctx};
    GA_CHECK(sb.stage(bases, n * sizeof(Affine<F>), flags & GA_BASES_ON_DEVICE));
    GA_CHECK(ss.stage(scalars, n * 32, flags & GA_SCALARS_ON_DEVICE));
    std::vector<XYZZ<F>> sums(want_windows ? win_hi - win_lo : 1);
    GA_CHECK((msm_run<C, G>(ctx, sb.dev, ss.dev, n, (flags & GA_SCALARS_MONTGOMERY) != 0, c, win_lo, win_hi, (size_t)ctx->tun.msm_max_chunk,
                            sums.data(), want_windows)));
    for (size_t w = 0; w < sums.size(); w++) host_store_jac<F>((char*)out + w * sizeof(Jac<F>), sums[w]);
    return GA_OK;
}

template <class C, int G>
int msm_table_create_run(MsmTable* t, const void* bases, unsigned flags) {
    typedef typename GroupField<C, G>::F F;
    Ctx* ctx = t->ctx;
    GA_CHECK(msm_plan_table<C>(t->n, &t->c, &t->nwin, (flags & GA_TABLE_BATCHED) != 0));
    t->bytes = (uint64_t)t->nwin * t->n * msm_table_point_bytes<C, G>();
    Staged sb{ctx};
    GA_CHECK(sb.stage(bases, t->n * sizeof(Affine<F>), flags & GA_BASES_ON_DEVICE));
    if (device_malloc(&t->d_table, t->bytes) != hipSuccess) {
        set_error("%s: device_malloc(%llu) failed", current_entry(), (unsigned long long)t->bytes);
        return GA_ERR_NOMEM;
    }
    GA_CHECK((msm_table_build<C, G>(ctx, sb.dev, t->n, t->c, t->d_table)));
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) {
        set_error("%s: table kernel failed", current_entry());
        return GA_ERR_HIP;
    }
    return GA_OK;
}

template <class C, int G>
int msm_table_run(MsmTable* t, const void* const* scalars, uint32_t k, unsigned flags, int win_lo, int win_hi, void* out_jacs) {
    typedef typename GroupField<C, G>::F F;
    Ctx* ctx = t->ctx;
    const bool mont = (flags & GA_SCALARS_MONTGOMERY) != 0;
    std::vector<Staged> st(k, Staged{ctx});   // (copies of an empty one; none is copied once it owns a buffer)
    std::vector<const void*> dev(k);
    for (uint32_t j = 0; j < k; j++) {
        GA_CHECK(st[j].stage(scalars[j], t->n * 32, flags & GA_SCALARS_ON_DEVICE));
        dev[j] = st[j].dev;
    }
    std::vector<XYZZ<F>> sums(k);
    if (k == 1) GA_CHECK((msm_table_device<C, G>(ctx, t->d_table, dev[0], t->n, mont, t->c, sums.data(), win_lo, win_hi)));
    else GA_CHECK((msm_table_device_batch<C, G>(ctx, t->d_table, dev.data(), (int)k, t->n, mont, t->c, sums.data())));
    for (uint32_t j = 0; j < k; j++) host_store_jac<F>((char*)out_jacs + j * sizeof(Jac<F>), sums[j]);
    return GA_OK;
}

// what msm_<curve>_g<k>.hip instantiates; the G1 unit of a curve has the group-independent half as well
#define GA_INSTANTIATE_MSM(C, G)                                                                                        \
    template int msm_run<C, G>(Ctx*, const void*, const void*, size_t, bool, int, int, int, size_t, void*, bool);       \
    template int msm_abi_run<C, G>(Ctx*, const void*, const void*, size_t, unsigned, int, int, void*, int*, int*, bool); \
    template int msm_table_create_run<C, G>(MsmTable*, const void*, unsigned);                                          \
    template int msm_table_run<C, G>(MsmTable*, const void* const*, uint32_t, unsigned, int, int, void*);               \
    template int msm_windows_device<C, G>(Ctx*, const void*, const void*, size_t, bool, int, int, int, void*, bool);    \
    template int msm_table_device<C, G>(Ctx*, const void*, const void*, size_t, bool, int, void*, int, int);            \
    template int msm_table_device_reuse<C, G>(Ctx*, const void*, const MsmPrepared&, void*);                            \
    template int msm_table_device_reuse_multi<C, G>(Ctx*, const void* const*, int, const MsmPrepared&, void*);          \
    template int msm_table_device_batch<C, G>(Ctx*, const void*, const void* const*, int, size_t, bool, int, void*);    \
    template int msm_table_build<C, G>(Ctx*, const void*, size_t, int, void*);                                          \
    template size_t msm_table_point_bytes<C, G>();
#define GA_INSTANTIATE_MSM_SCALARS(C) \
    template int msm_prepare_table_scalars<C>(Ctx*, const void*, size_t, bool, int, MsmPrepared*, int, int, int, int);

}  // namespace ga

// A sparse Fr matrix applied to a vector of curve points: out[row] = sum_k [coeff_k] points[col_k] over CSR rows -- the constraint loop
// of the Groth16 MPC ceremony's Phase2.Initialize (backend/groth16/<curve>/mpcsetup/phase2.go:224-247: A, B, B2, alpha B, beta A, C
// from the wire-major transposes of L, R, O over the Lagrange SRS), its K = beta A + alpha B + C (:283-300) over the concatenation
// [BetaTau | AlphaTau | Tau], and Z[i] = Tau[i + n] - Tau[i] (:256-261) as rows of two +-1 terms.
//
// Host, one walk over the matrix before anything is launched: row_start, every cid and every col are validated; every coefficient
// is classified by VALUE -- 0 (the term is dropped), +-1, +-2, or general with the magnitude min(c, r - c) and the sign moved to y
// (2^k and -2^k both get short ladders); every term becomes a code {kind | sign, operand index}; the general terms form the product
// list (row order, or sorted by coefficient id: GA_SPARSE_ORDER); rows are cut into segments of at most S terms (GA_SPARSE_SEGMENT).
//
// On the context's work stream, one host synchronisation (device-resident points and output):
//   1. products, GA_SPARSE_CHUNK general terms per pass:
//        sparse_gather_kernel          the pass's points and magnitudes, gathered side by side into scratch;
//        scale_points_window_kernel    the windowed ladder of scale_points.hip.h as it is: prod[g] = [|c|] points[col], packed hat XYZZ;
//        scale_points_exact_kernel     its flagged lanes with the complete formulas.
//   2. sparse_sums_kernel<F, true>     one lane per segment of terms.  The accumulator stays in registers and starts from the segment's
//                                      first operand that is not at infinity; every further one is ONE add29 of the affine point
//                                      (affine_to_lazy4), of its dbl29, or of prod[g], y negated (f29_sub<2>(0, y), before the
//                                      doubling: on a canonical value) for a minus sign.  Nothing is branched on inside the additions:
//                                      an exceptional one leaves ZZ == 0 (mod p), which is absorbing, so ONE exact test per segment
//                                      flags it.  A row of at most S terms writes its sum; a longer row writes partial sums, which
//      sparse_sums_kernel<F, false>    adds level by level (segments of at most S partials) until one sum per row remains: a row of
//                                      2^24 terms is six levels at S = 16.
//      sparse_sums_exact_kernel        the flagged segments of a level once more with the complete formulas of ec.hip.h, grid-stride
//                                      in one-wave workgroups; they count into `redone`.
//   3. fixed_base_affine_kernel (fixed_base.hip.h)  XYZZ -> affine, dense or at the bit-reversed row index.
// Bounds of the unreduced sequence: the two kernels use add29, dbl29, f29_sub<2>(0, y), from_mem and unpack only, and every operand
// is a canonical point, a negated one, or an output of add29 / dbl29 on such -- the closed set tools/lazy_bounds.py
// check_ladder(curve, fp2) bounds for G1 and G2.
#pragma once
#include <vector>

#include "csr_plan.hip.h"       // CsrLevels, csr_validate, csr_cut_levels; SPARSE_FINAL
#include "scale_points.hip.h"   // the windowed ladder and its exact redo; affine_to_lazy4, ec_ntt_pack / _unpack (ec_ntt.hip.h); vec_call.hip.h

namespace ga {

constexpr uint32_t SPARSE_DEFAULT_SEGMENT = 16;   // terms (or partial sums) per lane (GA_SPARSE_SEGMENT): the fastest whole call of the A/B over
                                                  // {8, 16, 32, 64, 128} on a matrix with one 2^20-term row (tools/phase2_init_bench.py)
// term code, word 0: kind in bits 0-1, bit 2 = subtract; word 1: the column (POINT, DOUBLE) or the product index (PRODUCT)
enum { SPARSE_SKIP = 0, SPARSE_POINT = 1, SPARSE_DOUBLE = 2, SPARSE_PRODUCT = 3, SPARSE_MINUS = 4 };

// the points and magnitudes of a pass of general terms, in the order of the product list
template <class F>
__global__ void __launch_bounds__(256)
sparse_gather_kernel(const Affine<F>* __restrict__ points, const uint32_t* __restrict__ gen, const uint32_t* __restrict__ mags, uint32_t n,
                     Affine<F>* __restrict__ gp, uint32_t* __restrict__ gs) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    store_pod(&gp[i], load_pod<Affine<F>>(&points[gen[2 * (uint64_t)i + 1]]));
    const uint64_t cid = gen[2 * (uint64_t)i];
#pragma unroll
    for (int k = 0; k < 8; k++) gs[(uint64_t)i * 8 + k] = mags[cid * 8 + k];
}

// operand k of a level: false when it is dropped (a zero coefficient, a point or a sum at infinity)
template <class F, bool TERMS>
__device__ __forceinline__ bool sparse_operand(const uint32_t* __restrict__ codes, const Affine<F>* __restrict__ points, const XYZZ<F>* __restrict__ in,
                                               uint64_t k, Lazy4<F>& e) {
    uint32_t kind = SPARSE_PRODUCT, minus = 0;
    uint64_t idx = k;
    if (TERMS) {
        const uint32_t code = codes[2 * k];
        kind = code & 3u;
        minus = code & SPARSE_MINUS;
        idx = codes[2 * k + 1];
        if (kind == SPARSE_SKIP) return false;
    }
    if (kind == SPARSE_PRODUCT) {
        const XYZZ<F> q = load_pod<XYZZ<F>>(&in[idx]);
        if (is_inf(q)) return false;
        e = ec_ntt_unpack<F>(q);
    } else {
        const Affine<F> P = load_pod<Affine<F>>(&points[idx]);
        if (is_inf(P)) return false;
        e = affine_to_lazy4<F>(P);
    }
    if (minus) e.y = f29_sub<2>(Lazy<F>::from_mem(FieldTraits<F>::zero()), e.y);   // 2p - y
    if (kind == SPARSE_DOUBLE) dbl29<F>(e);
    return true;
}

// segs: {first operand, operands, destination} per segment.  TERMS: the operands are term codes over points and products (`in`);
// otherwise they are the partial sums in[first ..] of the level before
template <class F, bool TERMS>
__global__ void __launch_bounds__(Table29<F>::THREADS, ScaleLadder<F>::MIN_WAVES)
sparse_sums_kernel(const uint32_t* __restrict__ segs, uint32_t nseg, const uint32_t* __restrict__ codes, const Affine<F>* __restrict__ points,
                   const XYZZ<F>* __restrict__ in, XYZZ<F>* __restrict__ part, XYZZ<F>* __restrict__ sums, uint32_t* __restrict__ redo,
                   uint32_t* __restrict__ redo_count) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nseg; i += gridDim.x * blockDim.x) {
        const uint64_t first = segs[3 * (uint64_t)i];
        const uint32_t count = segs[3 * (uint64_t)i + 1], dst = segs[3 * (uint64_t)i + 2];
        XYZZ<F>* out = (dst & SPARSE_FINAL) ? &sums[dst & ~SPARSE_FINAL] : &part[dst];
        Lazy4<F> acc;
        uint32_t k = 0;
        bool have = false;
        while (k < count && !have) have = sparse_operand<F, TERMS>(codes, points, in, first + k++, acc);
#pragma unroll 1
        for (; k < count; k++) {
            Lazy4<F> e;
            if (sparse_operand<F, TERMS>(codes, points, in, first + k, e)) add29<F>(acc, e);
        }
        if (!have) scale_store_inf<F>(out);
        else if (f29_is_zero_mod_p(acc.zz)) redo[atomicAdd(redo_count, 1u)] = i;
        else store_pod(out, ec_ntt_pack<F>(acc));
    }
}

// the flagged segments of a level with the complete formulas; lane 0 adds their number to the call's total (the kernels of a call run
// one after the other on one stream)
template <class F, bool TERMS>
__global__ void __launch_bounds__(64)
sparse_sums_exact_kernel(const uint32_t* __restrict__ segs, const uint32_t* __restrict__ codes, const Affine<F>* __restrict__ points,
                         const XYZZ<F>* __restrict__ in, XYZZ<F>* __restrict__ part, XYZZ<F>* __restrict__ sums, const uint32_t* __restrict__ redo,
                         const uint32_t* __restrict__ redo_count, uint64_t* __restrict__ total) {
    const uint32_t nredo = *redo_count;
    if (blockIdx.x == 0 && threadIdx.x == 0) *total += nredo;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < nredo; r += gridDim.x * blockDim.x) {
        const uint64_t i = redo[r];
        const uint64_t first = segs[3 * i];
        const uint32_t count = segs[3 * i + 1], dst = segs[3 * i + 2];
        XYZZ<F> acc = xyzz_inf<F>();
        for (uint32_t k = 0; k < count; k++) {
            uint32_t kind = SPARSE_PRODUCT, minus = 0;
            uint64_t idx = first + k;
            if (TERMS) {
                const uint32_t code = codes[2 * (first + k)];
                kind = code & 3u;
                minus = code & SPARSE_MINUS;
                idx = codes[2 * (first + k) + 1];
                if (kind == SPARSE_SKIP) continue;
            }
            XYZZ<F> e = kind == SPARSE_PRODUCT ? ec_ntt_to_exact<F>(load_pod<XYZZ<F>>(&in[idx])) : to_xyzz(load_pod<Affine<F>>(&points[idx]));
            if (kind == SPARSE_DOUBLE) e = dbl(e);
            if (minus) e = neg(e);
            acc = add(acc, e);
        }
        store_pod((dst & SPARSE_FINAL) ? &sums[dst & ~SPARSE_FINAL] : &part[dst], ec_ntt_from_exact<F>(acc));
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// what the walk over the matrix leaves for the device
struct SparsePlan {
    std::vector<uint32_t> codes;   // 2 words per term
    std::vector<uint32_t> gen;     // {cid, col} per general term, in product order
    std::vector<uint32_t> mags;    // 8 words per coefficient: min(c, r - c), canonical
    CsrLevels rows;                // the segments of the row sums, level after level
};

// coefficient -> (kind, minus); the magnitude into mag[8]
template <class FrP>
inline uint32_t sparse_classify(const void* coeff, bool mont, uint32_t* mag) {
    Fe<FrP> c;
    memcpy(&c, coeff, 32);
    if (mont) c = from_mont(c);
    else
        for (int k = 0; k < 6; k++) reduce_once<FrP>(c.l);   // any 256-bit integer: below r after at most 2^256 / r < 6 steps
    const Fe<FrP> m = neg(c);                                 // r - c (0 for c = 0)
    bool minus = false;
    for (int k = 7; k >= 0; k--)
        if (m.l[k] != c.l[k]) {
            minus = m.l[k] < c.l[k];
            break;
        }
    const Fe<FrP>& a = minus ? m : c;
    uint32_t high = 0;
    for (int k = 0; k < 8; k++) {
        mag[k] = a.l[k];
        if (k) high |= a.l[k];
    }
    if (high == 0 && a.l[0] == 0) return SPARSE_SKIP;
    const uint32_t kind = high == 0 && a.l[0] == 1 ? SPARSE_POINT : high == 0 && a.l[0] == 2 ? SPARSE_DOUBLE : SPARSE_PRODUCT;
    return kind | (minus ? SPARSE_MINUS : 0);
}

template <class C>
int sparse_sums_plan(size_t n_points, const uint64_t* row_start, size_t n_rows, const uint32_t* terms, const void* coeffs, size_t n_coeffs,
                     bool mont, uint32_t S, int cid_order, SparsePlan& plan) {
    typedef typename C::FrP FrP;
    GA_CHECK(csr_validate("ga_sparse_point_sums", "points", n_points, row_start, n_rows, terms, n_coeffs));
    const uint64_t nnz = row_start[n_rows];
    plan.mags.resize(n_coeffs * 8);
    std::vector<uint32_t> cls(n_coeffs);
    for (size_t i = 0; i < n_coeffs; i++) cls[i] = sparse_classify<FrP>((const char*)coeffs + i * 32, mont, &plan.mags[i * 8]);
    // product order: the position of every general term, by row or by coefficient id (a counting sort, stable in the rows)
    std::vector<uint64_t> next(cid_order ? n_coeffs + 1 : 1, 0);
    if (cid_order) {
        for (uint64_t k = 0; k < nnz; k++)
            if ((cls[terms[2 * k]] & 3u) == SPARSE_PRODUCT) next[terms[2 * k] + 1]++;
        for (size_t i = 0; i < n_coeffs; i++) next[i + 1] += next[i];
    }
    plan.codes.resize(2 * nnz);
    for (uint64_t k = 0; k < nnz; k++) {
        const uint32_t cid = terms[2 * k], col = terms[2 * k + 1], code = cls[cid];
        plan.codes[2 * k] = code;
        if ((code & 3u) == SPARSE_PRODUCT) {
            const uint64_t g = next[cid_order ? cid : 0]++;
            if (plan.gen.size() < 2 * (g + 1)) plan.gen.resize(2 * (g + 1));
            plan.gen[2 * g] = cid;
            plan.gen[2 * g + 1] = col;
            plan.codes[2 * k + 1] = (uint32_t)g;
        } else
            plan.codes[2 * k + 1] = col;
    }
    csr_cut_levels(row_start, n_rows, S, plan.rows);
    return GA_OK;
}

// segment: GA_SPARSE_SEGMENT (0 = default); cid_order: GA_SPARSE_ORDER; forced_chunk: GA_SPARSE_CHUNK (0 = default)
template <class C, int G>
int sparse_sums_run(Ctx* ctx, const void* points, size_t n_points, const uint64_t* row_start, size_t n_rows, const uint32_t* terms, const void* coeffs,
                    size_t n_coeffs, unsigned flags, void* out, uint64_t* redone, uint64_t forced_chunk, uint32_t segment, int cid_order) {
    typedef typename GroupField<C, G>::F F;
    const bool i_dev = (flags & GA_BASES_ON_DEVICE) != 0, o_dev = (flags & GA_RESULT_ON_DEVICE) != 0;
    const uint32_t S = segment >= 2 ? segment : SPARSE_DEFAULT_SEGMENT;
    SparsePlan plan;
    GA_CHECK(sparse_sums_plan<C>(n_points, row_start, n_rows, terms, coeffs, n_coeffs, (flags & GA_SCALARS_MONTGOMERY) != 0, S, cid_order, plan));
    const uint64_t nnz = plan.codes.size() / 2, ngen = plan.gen.size() / 2;
    const std::vector<uint32_t>& h_segs = plan.rows.segs;
    const uint64_t chunk = clamp_chunk(forced_chunk, SCALE_DEFAULT_CHUNK, ngen);
    uint64_t parts[2], max_seg = chunk;   // max_seg: the longest redo list, of a pass of products or of a level of segments
    plan.rows.part_sizes(parts);
    for (const CsrLevels::Level& lv : plan.rows.levels)
        if (lv.nseg > max_seg) max_seg = lv.nseg;
    const int logn = (flags & GA_RESULT_BITREVERSED) ? ilog2_u64(n_rows) : -1;
    hipStream_t st = ctx->work_stream();

    // the scratch of the whole call first: an allocation failure leaves nothing in flight
    XYZZ<F>*table = nullptr, *prods = nullptr, *part[2] = {nullptr, nullptr}, *sums;
    uint32_t *codes, *segs, *gen = nullptr, *mags = nullptr, *gs = nullptr;
    RedoList redo;   // header: the call's total (64 bits), the launch's count, pad
    Affine<F>*d_points = nullptr, *d_out = nullptr, *gp = nullptr;
    GA_CHECK(ctx->scratch_get("sparse_codes", nnz * 8, (void**)&codes));
    GA_CHECK(ctx->scratch_get("sparse_segments", h_segs.size() * 4, (void**)&segs));
    GA_CHECK(ctx->scratch_get("sparse_sums", n_rows * sizeof(XYZZ<F>), (void**)&sums));
    GA_CHECK(redo.get(ctx, "sparse_redo", max_seg, 8));
    if (ngen) {
        GA_CHECK(ctx->scratch_get("sparse_general", ngen * 8, (void**)&gen));
        GA_CHECK(ctx->scratch_get("sparse_magnitudes", plan.mags.size() * 4, (void**)&mags));
        GA_CHECK(ctx->scratch_get("sparse_products", ngen * sizeof(XYZZ<F>), (void**)&prods));
        GA_CHECK(ctx->scratch_get("sparse_gathered", chunk * sizeof(Affine<F>), (void**)&gp));
        GA_CHECK(ctx->scratch_get("scale_canonical", chunk * 32, (void**)&gs));                          // (the ladder's own buffers: shared with
        GA_CHECK(ctx->scratch_get("scale_table", SCALE_TABLE * chunk * sizeof(XYZZ<F>), (void**)&table));   //  ga_scale_points, never used at once)
    }
    for (int b = 0; b < 2; b++)
        if (parts[b]) GA_CHECK(ctx->scratch_get(b ? "sparse_partial_b" : "sparse_partial_a", parts[b] * sizeof(XYZZ<F>), (void**)&part[b]));
    if (!i_dev) GA_CHECK(ctx->scratch_get("sparse_points", n_points * sizeof(Affine<F>), (void**)&d_points));
    if (!o_dev) GA_CHECK(ctx->scratch_get("sparse_out", n_rows * sizeof(Affine<F>), (void**)&d_out));
    uint64_t* total = (uint64_t*)redo.words;
    uint32_t *count = redo.words + 2, *list = redo.list;
    StreamDrain drain{st};

    uint64_t h_total = 0;
    GA_HIP_CHECK(hipMemsetAsync(total, 0, 8, st));
    if (nnz) GA_HIP_CHECK(hipMemcpyAsync(codes, plan.codes.data(), nnz * 8, hipMemcpyHostToDevice, st));
    GA_HIP_CHECK(hipMemcpyAsync(segs, h_segs.data(), h_segs.size() * 4, hipMemcpyHostToDevice, st));
    const Affine<F>* src;
    GA_CHECK(chunk_in(st, i_dev, (const Affine<F>*)points, 0, n_points, d_points, &src));

    constexpr unsigned T = Table29<F>::THREADS;
    if (ngen) {
        GA_HIP_CHECK(hipMemcpyAsync(gen, plan.gen.data(), ngen * 8, hipMemcpyHostToDevice, st));
        GA_HIP_CHECK(hipMemcpyAsync(mags, plan.mags.data(), plan.mags.size() * 4, hipMemcpyHostToDevice, st));
    }
    for (uint64_t done = 0; done < ngen; done += chunk) {
        const uint32_t cn = (uint32_t)(ngen - done < chunk ? ngen - done : chunk);
        GA_HIP_CHECK(hipMemsetAsync(count, 0, 8, st));
        StageTimer tm(ctx, "sparse_products");
        const unsigned blocks = capped_grid(cn, T, SCALE_MAX_BLOCKS), exact_blocks = capped_grid(cn, 64, EC_NTT_EXACT_MAX_BLOCKS);
        hipLaunchKernelGGL((sparse_gather_kernel<F>), dim3((cn + 255) / 256), dim3(256), 0, st, src, (const uint32_t*)(gen + 2 * done), (const uint32_t*)mags, cn, gp, gs);
        hipLaunchKernelGGL((scale_points_window_kernel<F>), dim3(blocks), dim3(T), 0, st, (const Affine<F>*)gp, (const uint32_t*)gs, cn, table, prods + done, list, count);
        hipLaunchKernelGGL((scale_points_exact_kernel<F>), dim3(exact_blocks), dim3(64), 0, st, (const Affine<F>*)gp, (const uint32_t*)gs, prods + done,
                           (const uint32_t*)list, (const uint32_t*)count, total);
        GA_KERNEL_CHECK();
    }
    for (size_t l = 0; l < plan.rows.levels.size(); l++) {
        const CsrLevels::Level& lv = plan.rows.levels[l];
        if (lv.nseg == 0) continue;
        char name[32];
        snprintf(name, sizeof(name), "sparse_sums_%02d", (int)l);
        GA_HIP_CHECK(hipMemsetAsync(count, 0, 8, st));
        StageTimer tm(ctx, name);
        const uint32_t* sg = segs + 3 * lv.first;
        const unsigned blocks = capped_grid(lv.nseg, T, SCALE_MAX_BLOCKS), exact_blocks = capped_grid(lv.nseg, 64, EC_NTT_EXACT_MAX_BLOCKS);
        XYZZ<F>* to = part[l & 1];
        if (l == 0) {
            hipLaunchKernelGGL((sparse_sums_kernel<F, true>), dim3(blocks), dim3(T), 0, st, sg, lv.nseg, (const uint32_t*)codes, src, (const XYZZ<F>*)prods, to, sums, list, count);
            hipLaunchKernelGGL((sparse_sums_exact_kernel<F, true>), dim3(exact_blocks), dim3(64), 0, st, sg, (const uint32_t*)codes, src, (const XYZZ<F>*)prods, to, sums,
                               (const uint32_t*)list, (const uint32_t*)count, total);
        } else {
            const XYZZ<F>* from = part[(l - 1) & 1];
            hipLaunchKernelGGL((sparse_sums_kernel<F, false>), dim3(blocks), dim3(T), 0, st, sg, lv.nseg, (const uint32_t*)nullptr, src, from, to, sums, list, count);
            hipLaunchKernelGGL((sparse_sums_exact_kernel<F, false>), dim3(exact_blocks), dim3(64), 0, st, sg, (const uint32_t*)nullptr, src, from, to, sums,
                               (const uint32_t*)list, (const uint32_t*)count, total);
        }
        GA_KERNEL_CHECK();
    }
    GA_CHECK(launch_to_affine<F>(ctx, st, "sparse_affine", sums, (uint32_t)n_rows, 0, logn, o_dev ? (Affine<F>*)out : d_out));
    GA_CHECK(chunk_out(st, o_dev, (Affine<F>*)out, 0, n_rows, d_out));
    GA_HIP_CHECK(hipMemcpyAsync(&h_total, total, 8, hipMemcpyDeviceToHost, st));
    GA_HIP_CHECK(hipStreamSynchronize(st));   // the one synchronisation of a call with everything on the device
    if (redone) *redone = h_total;
    return GA_OK;
}

// what sparse_sums_<curve>_g<k>.hip instantiates
#define GA_INSTANTIATE_SPARSE_SUMS(C, G)                                                                                                        \
    template int sparse_sums_run<C, G>(Ctx*, const void*, size_t, const uint64_t*, size_t, const uint32_t*, const void*, size_t, unsigned, void*, \
                                       uint64_t*, uint64_t, uint32_t, int);

}  // namespace ga

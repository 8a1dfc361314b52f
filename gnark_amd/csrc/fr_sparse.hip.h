// A sparse Fr matrix applied to a vector of Fr elements: out[row] = s_row * sum_k coeffs[cid_k] * x[col_k] over CSR rows -- the scalar
// side of groth16.Setup (backend/groth16/<curve>/setup.go:346-428 setupABC: A, B, C from the wire-major transposes of L, R, O over the
// Lagrange values L_i(tau); :142-178: K = (beta A + alpha B + C) / delta or / gamma as ONE matrix [L | R | O] over the concatenation
// [beta lag | alpha lag | lag] with a scale per row class).  The Fr twin of sparse_sums.hip.h, with the same memory image.
//
// Host, one walk over the matrix before anything is launched: row_start, every cid, every col and every row class are validated; rows
// are cut into segments of at most S terms (GA_FR_SPARSE_SEGMENT).  Nothing is classified by value: a Montgomery product costs what the
// classification would, and a zero coefficient contributes zero by arithmetic.  Coefficients and row scales become Montgomery images
// (below r) on the host: the tables are small and stay in cache on the device.
//
// On the context's work stream, one host synchronisation:
//   fr_sparse_kernel<FrP, true>    one lane per segment of terms, grid-stride over a capped grid.  The accumulator is ONE fully reduced
//                                  element in registers; every term is a gather of x[col] (32 B), one product and one addition.  A row of
//                                  at most S terms writes s_row * sum to `out`; a longer row writes partial sums, which
//   fr_sparse_kernel<FrP, false>   adds level by level (segments of at most S partials) until one sum per row remains; the last level
//                                  of a row applies s_row.
// Domains: with canonical input (no GA_SCALARS_MONTGOMERY) x is reduced below r and the product of a Montgomery coefficient with a
// canonical x is the canonical c * x, with Montgomery input it is the Montgomery image: sums, partial sums and the product with the
// (Montgomery) row scale stay in the domain of x, which is the domain of the output.  No conversion pass.
// Traffic per term: 8 B of term and 32 B of gathered x; the coefficient table and the 12 B per segment are cached / amortised.
#pragma once
#include <vector>

#include "csr_plan.hip.h"    // CsrLevels, csr_validate, csr_cut_levels; SPARSE_FINAL: one segment shape for both sparse calls
#include "fr_powers.hip.h"   // fr_canonical
#include "vec_call.hip.h"    // StreamDrain, capped_grid, chunk_in / chunk_out

namespace ga {

constexpr uint32_t FR_SPARSE_DEFAULT_SEGMENT = 32;   // terms (or partial sums) per lane (GA_FR_SPARSE_SEGMENT): the fastest whole call on both curves of the
                                                     // A/B over {8, 16, 32, 64} on a matrix with one 2^20-term row (tools/setup_scalars_bench.py)
constexpr unsigned FR_SPARSE_THREADS = 256;
constexpr unsigned FR_SPARSE_MAX_BLOCKS = 1024;   // workgroups of a launch (grid-stride beyond): four per CU

// segs: {first operand, operands, destination} per segment.  TERMS: the operands are {cid, col} pairs over coeffs and x (`in`);
// otherwise they are the partial sums in[first ..] of the level before
template <class FrP, bool TERMS>
__global__ void __launch_bounds__(FR_SPARSE_THREADS)
fr_sparse_kernel(const uint32_t* __restrict__ segs, uint32_t nseg, const uint32_t* __restrict__ terms, const uint32_t* __restrict__ coeffs,
                 const uint32_t* __restrict__ in, int mont, uint32_t* __restrict__ part, uint32_t* __restrict__ out,
                 const uint8_t* __restrict__ row_class, const uint32_t* __restrict__ scales) {
    typedef Fe<FrP> F;
    // (64-bit index: nseg < n_rows + nnz / S < 2^32 may be within one grid of 2^32, where a 32-bit stride would wrap)
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nseg; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t first = segs[3 * i];
        const uint32_t count = segs[3 * i + 1], dst = segs[3 * i + 2];
        F acc = fe_zero<FrP>();
#pragma unroll 1
        for (uint32_t k = 0; k < count; k++) {
            if (TERMS) {
                const uint64_t cid = terms[2 * (first + k)], col = terms[2 * (first + k) + 1];
                F x = load_pod<F>(in + col * 8);
                if (!mont) x = fr_canonical(x, 0);
                acc = add(acc, mul(load_pod<F>(coeffs + cid * 8), x));
            } else
                acc = add(acc, load_pod<F>(in + (first + k) * 8));
        }
        if (dst & SPARSE_FINAL) {
            const uint64_t row = dst & ~SPARSE_FINAL;
            if (row_class) acc = mul(load_pod<F>(scales + (uint64_t)row_class[row] * 8), acc);
            store_pod(out + row * 8, acc);
        } else
            store_pod(part + (uint64_t)dst * 8, acc);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// validation (nothing has been written when it fails), then the segments
inline int fr_sparse_plan(size_t n_cols, const uint64_t* row_start, size_t n_rows, const uint32_t* terms, size_t n_coeffs, const uint8_t* row_class,
                          size_t n_classes, uint32_t S, CsrLevels& plan) {
    GA_CHECK(csr_validate("ga_fr_sparse_matvec", "columns", n_cols, row_start, n_rows, terms, n_coeffs));
    if (row_class)
        for (size_t r = 0; r < n_rows; r++)
            if (row_class[r] >= n_classes) {
                set_error("ga_fr_sparse_matvec: row_class[%zu] = %u outside %zu classes", r, (unsigned)row_class[r], n_classes);
                return GA_ERR_INVALID;
            }
    csr_cut_levels(row_start, n_rows, S, plan);
    return GA_OK;
}

// n elements as the ABI takes them -> Montgomery images below r (host)
template <class FrP>
inline std::vector<uint32_t> fr_host_montgomery(const void* v, size_t n, bool mont) {
    std::vector<uint32_t> w(n * 8);
    for (size_t i = 0; i < n; i++) {
        Fe<FrP> e;
        memcpy(&e, (const char*)v + i * 32, 32);
        if (!mont) e = to_mont(fr_canonical(e, 0));
        memcpy(&w[i * 8], &e, 32);
    }
    return w;
}

// segment: GA_FR_SPARSE_SEGMENT (0 = default)
template <class C>
int fr_sparse_run(Ctx* ctx, const void* x, size_t n_cols, const uint64_t* row_start, size_t n_rows, const uint32_t* terms, const void* coeffs,
                  size_t n_coeffs, const uint8_t* row_class, const void* row_scales, size_t n_classes, unsigned flags, void* out, uint32_t segment) {
    typedef typename C::FrP FrP;
    const bool mont = (flags & GA_SCALARS_MONTGOMERY) != 0, i_dev = (flags & GA_BASES_ON_DEVICE) != 0, o_dev = (flags & GA_RESULT_ON_DEVICE) != 0;
    const uint32_t S = segment >= 2 ? segment : FR_SPARSE_DEFAULT_SEGMENT;
    CsrLevels plan;
    GA_CHECK(fr_sparse_plan(n_cols, row_start, n_rows, terms, n_coeffs, row_class, n_classes, S, plan));
    const uint64_t nnz = row_start[n_rows];
    const std::vector<uint32_t> h_coeffs = fr_host_montgomery<FrP>(coeffs, nnz ? n_coeffs : 0, mont);
    const std::vector<uint32_t> h_scales = fr_host_montgomery<FrP>(row_scales, row_class ? n_classes : 0, mont);
    uint64_t parts[2];
    plan.part_sizes(parts);
    hipStream_t st = ctx->work_stream();

    // the scratch of the whole call first: an allocation failure leaves nothing in flight
    uint32_t *d_terms = nullptr, *d_segs, *d_coeffs = nullptr, *d_scales = nullptr, *part[2] = {nullptr, nullptr}, *d_x = nullptr, *d_out = nullptr;
    uint8_t* d_class = nullptr;
    if (nnz) GA_CHECK(ctx->scratch_get("fr_sparse_terms", nnz * 8, (void**)&d_terms));
    GA_CHECK(ctx->scratch_get("fr_sparse_segments", plan.segs.size() * 4, (void**)&d_segs));
    if (nnz) GA_CHECK(ctx->scratch_get("fr_sparse_coeffs", h_coeffs.size() * 4, (void**)&d_coeffs));
    if (row_class) {
        GA_CHECK(ctx->scratch_get("fr_sparse_scales", h_scales.size() * 4, (void**)&d_scales));
        GA_CHECK(ctx->scratch_get("fr_sparse_classes", n_rows, (void**)&d_class));
    }
    for (int b = 0; b < 2; b++)
        if (parts[b]) GA_CHECK(ctx->scratch_get(b ? "fr_sparse_partial_b" : "fr_sparse_partial_a", parts[b] * 32, (void**)&part[b]));
    if (!i_dev && n_cols) GA_CHECK(ctx->scratch_get("fr_sparse_x", n_cols * 32, (void**)&d_x));
    if (!o_dev) GA_CHECK(ctx->scratch_get("fr_sparse_out", n_rows * 32, (void**)&d_out));
    StreamDrain drain{st};

    if (nnz) {
        GA_HIP_CHECK(hipMemcpyAsync(d_terms, terms, nnz * 8, hipMemcpyHostToDevice, st));
        GA_HIP_CHECK(hipMemcpyAsync(d_coeffs, h_coeffs.data(), h_coeffs.size() * 4, hipMemcpyHostToDevice, st));
    }
    GA_HIP_CHECK(hipMemcpyAsync(d_segs, plan.segs.data(), plan.segs.size() * 4, hipMemcpyHostToDevice, st));
    if (row_class) {
        GA_HIP_CHECK(hipMemcpyAsync(d_scales, h_scales.data(), h_scales.size() * 4, hipMemcpyHostToDevice, st));
        GA_HIP_CHECK(hipMemcpyAsync(d_class, row_class, n_rows, hipMemcpyHostToDevice, st));
    }
    const uint32_t* src;
    GA_CHECK(chunk_in(st, i_dev, (const uint32_t*)x, 0, n_cols * 8, d_x, &src));
    uint32_t* dst = o_dev ? (uint32_t*)out : d_out;

    for (size_t l = 0; l < plan.levels.size(); l++) {
        const CsrLevels::Level& lv = plan.levels[l];
        if (lv.nseg == 0) continue;
        char name[32];
        snprintf(name, sizeof(name), "fr_sparse_%02d", (int)l);
        StageTimer tm(ctx, name);
        const uint32_t* sg = d_segs + 3 * lv.first;
        const unsigned blocks = capped_grid(lv.nseg, FR_SPARSE_THREADS, FR_SPARSE_MAX_BLOCKS);
        if (l == 0)
            hipLaunchKernelGGL((fr_sparse_kernel<FrP, true>), dim3(blocks), dim3(FR_SPARSE_THREADS), 0, st, sg, lv.nseg, (const uint32_t*)d_terms, (const uint32_t*)d_coeffs, src,
                               (int)mont, part[0], dst, (const uint8_t*)d_class, (const uint32_t*)d_scales);
        else
            hipLaunchKernelGGL((fr_sparse_kernel<FrP, false>), dim3(blocks), dim3(FR_SPARSE_THREADS), 0, st, sg, lv.nseg, (const uint32_t*)nullptr, (const uint32_t*)nullptr,
                               (const uint32_t*)part[(l - 1) & 1], (int)mont, part[l & 1], dst, (const uint8_t*)d_class, (const uint32_t*)d_scales);
        GA_KERNEL_CHECK();
    }
    GA_CHECK(chunk_out(st, o_dev, (uint32_t*)out, 0, n_rows * 8, d_out));
    GA_HIP_CHECK(hipStreamSynchronize(st));   // the one synchronisation of a call with everything on the device
    return GA_OK;
}

// what fr_setup_<curve>.hip instantiates, with GA_INSTANTIATE_FR_SETUP (fr_setup.hip.h)
#define GA_INSTANTIATE_FR_SPARSE(C)                                                                                                          \
    template int fr_sparse_run<C>(Ctx*, const void*, size_t, const uint64_t*, size_t, const uint32_t*, const void*, size_t, const uint8_t*, \
                                  const void*, size_t, unsigned, void*, uint32_t);

}  // namespace ga

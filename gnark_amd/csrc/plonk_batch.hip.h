// The three PLONK-specific drivers, each for `count` proofs of one circuit per device pass: the grand product (ga_plonk_build_z,
// ga_plonk_build_z_batch), the quotient over a pinned key (ga_plonk_quotient_pinned, ga_plonk_quotient_pinned_batch) and the
// division of kzg.Open (ga_kzg_open, ga_fr_poly_evaluate, ga_kzg_open_batch).  The single calls are count = 1 (the wrappers of
// common.hip.h, and count = 1 of kzg_open_run at the end of this file): there is no second implementation.  The proof is the grid's y dimension (or a segment of a flat index), the per-proof
// challenges come from a device array uploaded once per pass, every power table is built on the device, the scans are segmented per
// proof, and a pass of up to PLONK_BATCH_LIMIT proofs of the grand product or the quotient ends in ONE synchronisation (a division
// pass has none: its caller synchronises).  The kernels are those of plonk.hip.h.
// Every stored field element is fully reduced, so row j of every output is the same bit for bit however the proofs are split into
// passes and whatever the association order of the scans.
#pragma once
#include "hostops.hip.h"    // host_store_jac
#include "plonk.hip.h"
#include "vec_call.hip.h"   // Staged, StreamDrain

namespace ga {

// ---- grand product ---------------------------------------------------------------------------------------------------------------
// iop.BuildRatioCopyConstraint for `count` proofs of one circuit: Z in Lagrange form (regular layout) from L, R, O (Lagrange regular)
// and the permutation; L, R, O, z_out = [count][n], betas / gammas = count host elements.
// Aliasing: device operands are read in place, by the ratio-terms launch alone, and row j of z_out is written by the last launch of
// the pass that holds proof j -- after that pass's only read of row j of L, R and O, on the one stream.  So z_out may be the very
// buffer of L, R or O (the same base address: row j then overwrites the row j it was computed from); a z_out that overlaps an input
// at any other offset is not supported.  Host operands are staged, and z_out is written after the pass has read them.
template <class FrP>
int plonk_build_z(Domain* d0, const void* L, const void* R, const void* O, const int64_t* perm, const void* betas, const void* gammas,
                  uint32_t count, PlonkBatchKnobs knobs, bool on_device, void* z_out) {
    typedef Fe<FrP> F;
    Ctx* ctx = d0->ctx;
    const uint64_t n = d0->n;
    hipStream_t st = ctx->stream;
    const hipMemcpyKind kin = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    int64_t* dperm;
    GA_CHECK(ctx->scratch_get("plonk_zb_perm", 3 * n * 8, (void**)&dperm));
    GA_HIP_CHECK(hipMemcpyAsync(dperm, perm, 3 * n * 8, kin, st));
    if (on_device) {   // a host permutation was range-checked by the entry point
        uint32_t* d_bad;
        GA_CHECK(ctx->scratch_get("plonk_perm_bad", 256, (void**)&d_bad));
        GA_HIP_CHECK(hipMemsetAsync(d_bad, 0, 4, st));
        hipLaunchKernelGGL(plonk_perm_check_kernel, dim3((unsigned)((3 * n + 255) / 256)), dim3(256), 0, st, (const int64_t*)dperm, 3 * n, d_bad);
        GA_KERNEL_CHECK();
        uint32_t bad = 0;
        GA_HIP_CHECK(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st));
        GA_HIP_CHECK(hipStreamSynchronize(st));
        if (bad) {
            set_error("%s: %u entries of the device-resident permutation are outside [0, 3n)", current_entry(), bad);
            return GA_ERR_INVALID;
        }
    }
    uint32_t *lro = nullptr, *num = nullptr, *den = nullptr, *tmp = nullptr, *z = nullptr, *cp = nullptr, *cst = nullptr;
    // The chunk of the prefix product is chosen ONCE, for the pass size the scratch was reserved for, and kept by every pass: a later,
    // smaller pass then has fewer chunk products than were reserved (plonk_scan_chunk is not monotone in its total: chosen per pass,
    // nine proofs of 2^13 take chunks of 16 and the eight that follow chunks of 8 -- twice the chunk products).  A power of two no larger
    // than n: it divides n, so no chunk spans two proofs, and a proof smaller than one chunk is its own chunk.
    uint64_t chunk = 0;
    auto reserve = [&](uint32_t cnt) -> int {
        const size_t rows = (size_t)cnt * n * 32;
        chunk = plonk_scan_chunk((uint64_t)cnt * n, knobs.scan_threads);
        if (chunk > n) chunk = n;
        GA_CHECK(ctx->scratch_get("plonk_zb_lro", on_device ? 256 : 3 * rows, (void**)&lro));
        GA_CHECK(ctx->scratch_get("plonk_zb_num", rows, (void**)&num));
        GA_CHECK(ctx->scratch_get("plonk_zb_den", rows, (void**)&den));
        GA_CHECK(ctx->scratch_get("plonk_zb_tmp", rows, (void**)&tmp));
        GA_CHECK(ctx->scratch_get("plonk_zb_out", on_device ? 256 : rows, (void**)&z));
        GA_CHECK(ctx->scratch_get("plonk_zb_chunks", rows / chunk, (void**)&cp));
        GA_CHECK(ctx->scratch_get("plonk_zb_consts", (size_t)cnt * 64 + 64, (void**)&cst));
        return GA_OK;
    };
    // the identity table w^j (once per call) and the coset shifts of the three wire columns
    const F g = fe_const<FrP>(FrP::GEN);
    std::vector<uint32_t> wstage;
    pow_pair<FrP>(wstage, plonk_ld<FrP>(d0->w), fe_one<FrP>());
    PowTables<FrP> wt;
    GA_CHECK(wt.build(ctx, "plonk_zb_wtab", wstage, 1, n));
    std::vector<uint32_t> hc;   // per pass: [shift, shift^2][beta, gamma] x cnt; alive until the pass has synchronised
    auto pass = [&](uint32_t first, uint32_t cnt) -> int {
        const size_t off = (size_t)first * n * 32, rows = (size_t)cnt * n * 32;
        const uint64_t total = (uint64_t)cnt * n;
        const uint32_t *dl = (const uint32_t*)((const char*)L + off), *dr = (const uint32_t*)((const char*)R + off),
                       *dO = (const uint32_t*)((const char*)O + off);
        uint32_t* dz = on_device ? (uint32_t*)((char*)z_out + off) : z;
        if (!on_device) {
            const void* src[3] = {dl, dr, dO};
            for (int k = 0; k < 3; k++) GA_HIP_CHECK(hipMemcpyAsync(lro + (size_t)k * total * 8, src[k], rows, hipMemcpyHostToDevice, st));
            dl = lro, dr = lro + total * 8, dO = lro + 2 * total * 8;
        }
        hc.assign(16 + (size_t)cnt * 16, 0);
        memcpy(&hc[0], g.l, 32);
        const F gg = sqr(g);
        memcpy(&hc[8], gg.l, 32);
        for (uint32_t j = 0; j < cnt; j++) {
            memcpy(&hc[16 + (size_t)j * 16], (const char*)betas + (size_t)(first + j) * 32, 32);
            memcpy(&hc[24 + (size_t)j * 16], (const char*)gammas + (size_t)(first + j) * 32, 32);
        }
        GA_HIP_CHECK(hipMemcpyAsync(cst, hc.data(), hc.size() * 4, hipMemcpyHostToDevice, st));
        {
            StageTimer tm(ctx, "plonk_zb_terms");
            hipLaunchKernelGGL((plonk_ratio_terms_kernel<FrP>), dim3((unsigned)((n + 255) / 256), cnt), dim3(256), 0, st, dl, dr, dO,
                               (const int64_t*)dperm, wt.lo(0), wt.hi(0), NTT_POW_LO_BITS, cst + 16, cst, num, den, n);
            GA_KERNEL_CHECK();
        }
        {
            StageTimer tm(ctx, "plonk_zb_batch_inverse");
            const uint64_t threads = plonk_inverse_threads(total);
            hipLaunchKernelGGL((fr_batch_inverse_kernel<FrP>), dim3((unsigned)((threads + 63) / 64)), dim3(64), 0, st, den, tmp, total);
            GA_KERNEL_CHECK();
        }
        {
            StageTimer tm(ctx, "plonk_zb_prefix_product");
            const uint64_t nchunks = total / chunk;   // <= the reserved pass's: cnt <= its size, the chunk is the same
            const unsigned cb = (unsigned)((nchunks + 63) / 64);
            hipLaunchKernelGGL((fr_chunk_product_kernel<FrP>), dim3(cb), dim3(64), 0, st, num, den, cp, total, chunk);
            hipLaunchKernelGGL((fr_chunk_scan_kernel<FrP>), dim3(1, cnt), dim3(256), 0, st, cp, n / chunk);
            hipLaunchKernelGGL((fr_chunk_apply_kernel<FrP>), dim3(cb), dim3(64), 0, st, num, den, cp, dz, total, chunk);
            GA_KERNEL_CHECK();
        }
        if (!on_device) GA_HIP_CHECK(hipMemcpyAsync((char*)z_out + off, z, rows, hipMemcpyDeviceToHost, st));
        GA_HIP_CHECK(hipStreamSynchronize(st));
        return GA_OK;
    };
    const int rc = plonk_batch_chunks(count, knobs.batch_max, reserve, pass);
    if (rc != GA_OK) hipStreamSynchronize(st);   // the staging vectors above die at return: no copy from them may still be queued
    return rc;
}

// ---- quotient over a pinned key ----------------------------------------------------------------------------------------------------
// The per-proof polynomials only; the constraints read the circuit constants and 1/(x-1) from the key.
// args[0 .. count): the per-proof polynomials of `count` proofs (one nb_bsb, one lagrange_mask, one on_device); h_out = [count][rho * n]
template <class FrP>
int plonk_quotient_pinned(PlonkFixed* fx, const PlonkQuotientArgs* args, uint32_t count, PlonkBatchKnobs knobs, void* h_out) {
    Domain *d0 = fx->d0, *d1 = fx->d1;
    Ctx* ctx = d0->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t n = d0->n;
    const PlonkQuotientArgs& A0 = args[0];
    if (fx->nb_bsb != A0.nb_bsb) {
        set_error("plonk quotient: the pinned key was built for %u BSB22 gates", fx->nb_bsb);
        return GA_ERR_INVALID;
    }
    PlonkCosets<FrP> cosets;   // alive until the last pass has synchronised
    int rc = cosets.build(d0, d1, A0.nb_bsb);
    const uint64_t rho = cosets.rho;
    const int np = PLONK_NB_FIXED + 2 * (int)A0.nb_bsb;
    // the per-proof ids, those given as evaluations first: slot s holds [cnt][n], so the inverse transforms are the first nlag * cnt
    // vectors of the canonical buffer and the bit-reversing copies the rest
    std::vector<int> ids;
    for (int lag = 1; lag >= 0; lag--)
        for (int p : plonk_ids(np, false))
            if ((int)((A0.lagrange_mask >> p) & 1) == lag) ids.push_back(p);
    const uint64_t k = ids.size();
    uint64_t nlag = 0;
    for (int p : ids) nlag += (A0.lagrange_mask >> p) & 1;
    uint32_t *canon = nullptr, *work = nullptr, *cres = nullptr;
    PlonkConsts* dK = nullptr;
    auto reserve = [&](uint32_t cnt) -> int {
        GA_CHECK(ctx->scratch_get("plonk_qb_canon", (size_t)cnt * k * n * 32, (void**)&canon));
        GA_CHECK(ctx->scratch_get("plonk_qb_work", (size_t)cnt * k * n * 32, (void**)&work));
        GA_CHECK(ctx->scratch_get("plonk_qb_cres", (size_t)cnt * d1->n * 32, (void**)&cres));
        GA_CHECK(ctx->scratch_get("plonk_qb_consts", (size_t)cnt * rho * sizeof(PlonkConsts), (void**)&dK));
        return GA_OK;
    };
    std::vector<PlonkConsts> hK;   // [rho][cnt]; alive until the pass has synchronised
    auto pass = [&](uint32_t first, uint32_t cnt) -> int {
        const PlonkQuotientArgs* A = args + first;
        const hipMemcpyKind kin = A0.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        auto vec = [&](uint32_t* base, uint64_t s, uint32_t j) { return base + ((size_t)s * cnt + j) * n * 8; };
        {
            StageTimer tm(ctx, "plonk_qb_h2d");
            for (uint64_t s = 0; s < k; s++)
                for (uint32_t j = 0; j < cnt; j++)
                    GA_HIP_CHECK(hipMemcpyAsync(vec(s < nlag ? canon : work, s, j), A[j].polys[ids[s]], n * 32, kin, st));
        }
        // the constants of every (coset, proof)
        hK.resize((size_t)rho * cnt);
        for (uint64_t i = 0; i < rho; i++)
            for (uint32_t j = 0; j < cnt; j++) {
                hK[i * cnt + j] = cosets.K[i];
                plonk_proof_consts<FrP>(hK[i * cnt + j], A[j], cosets.cexp[i]);
            }
        GA_HIP_CHECK(hipMemcpyAsync(dK, hK.data(), hK.size() * sizeof(PlonkConsts), hipMemcpyHostToDevice, st));
        // to canonical coefficients in bit-reversed order: one inverse DIF over the evaluation vectors (p.ToCanonical, prove.go:1036),
        // one bit-reversing copy over the coefficient vectors
        if (nlag) GA_CHECK(ntt_run<FrP>(d0, canon, /*inverse=*/true, /*dit=*/false, scale_none(), scale_const(d0->ninv), nullptr, nullptr, nlag * cnt));
        if (k > nlag) {
            StageTimer tm(ctx, "plonk_qb_bitrev");
            hipLaunchKernelGGL((fr_bitrev_copy_kernel<FrP>), dim3((unsigned)((n + 255) / 256), (unsigned)((k - nlag) * cnt)), dim3(256), 0, st,
                               vec(canon, nlag, 0), vec(work, nlag, 0), n, d0->logn);
            GA_KERNEL_CHECK();
        }
        PlonkBatchPtrs B;
        memset(&B, 0, sizeof(B));
        B.P.nb_bsb = (int)A0.nb_bsb;
        B.stride = n * 8;
        for (uint64_t s = 0; s < k; s++) {
            B.P.p[ids[s]] = vec(work, s, 0);
            B.proofs |= 1ull << ids[s];
        }
        for (uint64_t i = 0; i < rho; i++) {
            // ONE out-of-place coset transform over every per-proof polynomial of the pass
            GA_CHECK(ntt_run<FrP>(d0, work, /*inverse=*/false, /*dit=*/true, scale_none(), scale_none(), canon, cosets.tw[i], k * cnt));
            for (int p : plonk_ids(np, true)) B.P.p[p] = fx->evals_of(i, p);
            StageTimer tm(ctx, "plonk_qb_constraints");
            hipLaunchKernelGGL((plonk_constraints_kernel<FrP, PLONK_LAZY<FrP>>), dim3((unsigned)((n + 127) / 128), cnt), dim3(128), 0, st, B,
                               (const PlonkConsts*)(dK + i * cnt), cosets.x.lo(i), cosets.x.hi(i), NTT_POW_LO_BITS, fx->inv_xm1_of(i),
                               cres + cosets.block(i) * n * 8, d1->n * 8, n, d0->logn);
            GA_KERNEL_CHECK();
        }
        // ONE inverse coset transform of size rho * n over the pass (prove.go:1319), then the h leave together
        GA_CHECK(ntt_fft<FrP>(d1, cres, GA_FFT_INVERSE, GA_DIT, 1, cnt));
        {
            StageTimer tm(ctx, "plonk_qb_d2h");
            GA_HIP_CHECK(hipMemcpyAsync((char*)h_out + (size_t)first * d1->n * 32, cres, (size_t)cnt * d1->n * 32,
                                        A0.on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
        }
        GA_HIP_CHECK(hipStreamSynchronize(st));
        return GA_OK;
    };
    if (rc == GA_OK) rc = plonk_batch_chunks(count, knobs.batch_max, reserve, pass);
    if (rc != GA_OK) hipStreamSynchronize(st);   // the staging vectors above die at return: no copy from them may still be queued
    return rc;
}

// ---- kzg.Open's division -------------------------------------------------------------------------------------------------------------
// One pass: (p_j(X) - p_j(z_j)) / (X - z_j) for count <= PLONK_BATCH_LIMIT polynomials of n >= 1 coefficients (the kernels of
// plonk.hip.h: scaling by z_j^i, suffix sum, scaling by z_j^-(k+1), or a shifted copy where z_j = 0).  Nothing is synchronised here.
template <class FrP>
int kzg_divide_by_linear(Ctx* ctx, const void* const* d_polys, uint64_t n, uint32_t count, const void* points, uint32_t* d_quot,
                         uint64_t quot_stride, uint32_t* d_values, uint64_t scan_threads, std::vector<uint32_t>& stage) {
    typedef Fe<FrP> F;
    hipStream_t st = ctx->stream;
    if (count == 0 || count > PLONK_BATCH_LIMIT || n == 0 || quot_stride < n) {
        set_error("kzg division: 1 .. %u polynomials of at least one coefficient per pass", PLONK_BATCH_LIMIT);
        return GA_ERR_INVALID;
    }
    KzgBatchPtrs in;
    memset(&in, 0, sizeof(in));
    // the tables z_j^i and z_j^-i of every item, built on the device from one upload of the 2 * count bases out of the caller's
    // `stage`, which lives until the caller has synchronised the stream
    stage.clear();
    for (uint32_t j = 0; j < count; j++) {
        in.p[j] = (const uint32_t*)d_polys[j];
        const F z = plonk_ld<FrP>(points, (int)j);
        pow_pair<FrP>(stage, z, fe_one<FrP>());
        pow_pair<FrP>(stage, inv(z), fe_one<FrP>());
    }
    const uint64_t chunk = plonk_scan_chunk((uint64_t)count * n, scan_threads), cpp = (n + chunk - 1) / chunk, nchunks = cpp * count;
    uint32_t *t, *cs;
    GA_CHECK(ctx->scratch_get("kzg_b_t", (size_t)count * n * 32, (void**)&t));
    GA_CHECK(ctx->scratch_get("kzg_b_chunks", nchunks * 32, (void**)&cs));
    StageTimer tm(ctx, "kzg_b_divide");
    PowTables<FrP> pt;
    GA_CHECK(pt.build(ctx, "kzg_b_tabs", stage, 2 * (uint64_t)count, n));
    const unsigned blocks = (unsigned)((n + 255) / 256), cb = (unsigned)((nchunks + 63) / 64);
    hipLaunchKernelGGL((kzg_scale_kernel<FrP>), dim3(blocks, count), dim3(256), 0, st, in, t, pt.tabs, pt.words, NTT_POW_LO_BITS, n);
    hipLaunchKernelGGL((fr_chunk_sum_kernel<FrP>), dim3(cb), dim3(64), 0, st, t, cs, n, chunk, cpp, nchunks);
    hipLaunchKernelGGL((fr_chunk_suffix_scan_kernel<FrP>), dim3(1, count), dim3(256), 0, st, cs, cpp);
    hipLaunchKernelGGL((fr_chunk_suffix_apply_kernel<FrP>), dim3(cb), dim3(64), 0, st, t, cs, n, chunk, cpp, nchunks);
    hipLaunchKernelGGL((kzg_quotient_kernel<FrP>), dim3(blocks, count), dim3(256), 0, st, in, (const uint32_t*)t,
                       (const uint32_t*)pt.bases, (const uint32_t*)pt.tabs, pt.words, NTT_POW_LO_BITS, n, d_quot,
                       quot_stride, d_values);
    GA_KERNEL_CHECK();
    return GA_OK;
}

// ---- the per-curve calls declared in common.hip.h: C::FrP for the drivers above ------------------------------------------------
template <class C>
int plonk_domain_build_z_batch(Domain* d0, const void* L, const void* R, const void* O, const int64_t* perm, const void* betas, const void* gammas,
                               uint32_t count, PlonkBatchKnobs knobs, bool on_device, void* z_out) {
    return plonk_build_z<typename C::FrP>(d0, L, R, O, perm, betas, gammas, count, knobs, on_device, z_out);
}
template <class C>
int plonk_domain_quotient_pinned_batch(PlonkFixed* fx, const PlonkQuotientArgs* args, uint32_t count, PlonkBatchKnobs knobs, void* h_out) {
    return plonk_quotient_pinned<typename C::FrP>(fx, args, count, knobs, h_out);
}
template <class C>
int kzg_domain_divide_batch(Ctx* ctx, const void* const* d_polys, uint64_t n, uint32_t count, const void* points, void* d_quot, uint64_t quot_stride,
                            void* d_values, uint64_t scan_threads, std::vector<uint32_t>* stage) {
    return kzg_divide_by_linear<typename C::FrP>(ctx, d_polys, n, count, points, (uint32_t*)d_quot, quot_stride, (uint32_t*)d_values, scan_threads, *stage);
}
// ga_fr_poly_evaluate: the division alone, for its value (the quotient lands in the batch path's quotient scratch and stays there)
template <class C>
int kzg_domain_divide(Ctx* ctx, const void* poly, uint64_t n, const void* z_mont, void* value_out, bool on_device, uint64_t scan_threads) {
    Staged sp{ctx};
    GA_CHECK(sp.stage(poly, n * 32, on_device));
    char *q, *d_value;
    GA_CHECK(ctx->scratch_get("kzg_b_quotient", n * 32, (void**)&q));
    GA_CHECK(ctx->scratch_get("kzg_b_values", 32, (void**)&d_value));
    std::vector<uint32_t> stage;   // the division's small upload: outlives the drain
    StreamDrain drain{ctx->stream};
    GA_HIP_CHECK(hipMemsetAsync(q + (n - 1) * 32, 0, 32, ctx->stream));
    GA_CHECK(kzg_domain_divide_batch<C>(ctx, &sp.dev, n, 1, z_mont, q, n, d_value, scan_threads, &stage));
    GA_HIP_CHECK(hipMemcpyAsync(value_out, d_value, 32, hipMemcpyDeviceToHost, ctx->stream));
    GA_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return GA_OK;
}

// kzg.Open for `count` polynomials of one length over one SRS: per pass of at most knobs.batch_max items the divisions by (X - z_j)
// are one launch chain and the quotients one batched table MSM, whose synchronisation (it returns its sums) ends the pass
template <class C>
int kzg_open_run(MsmTable* t, const void* const* polys, size_t n, uint32_t count, unsigned flags, const void* points, void* claimed_values_out,
                 void* h_out, PlonkBatchKnobs knobs) {
    typedef typename GroupField<C, GA_G1>::F F;
    Ctx* c = t->ctx;
    uint32_t batch_max = knobs.batch_max;
    while (batch_max > 1 && (uint64_t)batch_max * t->nwin * t->n >= (1ull << 31)) batch_max--;   // the pair index space of one batched MSM
    if ((uint64_t)batch_max * t->nwin * t->n >= (1ull << 31)) {
        set_error("%s: %d windows x %zu points exceed the 2^31 pair index space of the batched table MSM", current_entry(), t->nwin, (size_t)t->n);
        return GA_ERR_INVALID;
    }
    const bool on_device = (flags & GA_SCALARS_ON_DEVICE) != 0;
    const size_t qn = n > t->n ? n : t->n;   // a row of quotients: the table's n scalars (zero beyond the n - 1 coefficients)
    char *in = nullptr, *q = nullptr, *vals = nullptr;
    auto reserve = [&](uint32_t cnt) -> int {
        GA_CHECK(c->scratch_get("kzg_b_in", on_device ? 256 : (size_t)cnt * n * 32, (void**)&in));
        GA_CHECK(c->scratch_get("kzg_b_quotient", (size_t)cnt * qn * 32, (void**)&q));
        GA_CHECK(c->scratch_get("kzg_b_values", (size_t)cnt * 32, (void**)&vals));
        return GA_OK;
    };
    std::vector<XYZZ<F>> sums(PLONK_BATCH_LIMIT);
    std::vector<uint32_t> stage;   // the division's small upload; read before the MSM of its pass has returned
    StreamDrain drain{c->stream};  // `stage` and the caller's polynomials: no copy from them is still queued on any way out
    // (the division and the MSM get their own scratch inside the pass: plonk_batch_chunks halves a pass that fails there as well)
    auto pass = [&](uint32_t first, uint32_t cnt) -> int {
        const void *dpoly[PLONK_BATCH_LIMIT], *dquot[PLONK_BATCH_LIMIT];
        for (uint32_t j = 0; j < cnt; j++) {
            dpoly[j] = polys[first + j];
            if (!on_device) {
                GA_HIP_CHECK(hipMemcpyAsync(in + (size_t)j * n * 32, polys[first + j], n * 32, hipMemcpyHostToDevice, c->stream));
                dpoly[j] = in + (size_t)j * n * 32;
            }
            dquot[j] = q + (size_t)j * qn * 32;
        }
        GA_HIP_CHECK(hipMemsetAsync(q, 0, (size_t)cnt * qn * 32, c->stream));
        GA_CHECK(kzg_domain_divide_batch<C>(c, dpoly, n, cnt, (const char*)points + (size_t)first * 32, q, qn, vals, knobs.scan_threads, &stage));
        // the claimed values leave in one copy ahead of the MSM, whose synchronisation completes it
        GA_HIP_CHECK(hipMemcpyAsync((char*)claimed_values_out + (size_t)first * 32, vals, (size_t)cnt * 32, hipMemcpyDeviceToHost, c->stream));
        GA_CHECK((msm_table_device_batch<C, GA_G1>(c, t->d_table, dquot, (int)cnt, t->n, true, t->c, sums.data())));
        for (uint32_t j = 0; j < cnt; j++) host_store_jac<F>((char*)h_out + (size_t)(first + j) * sizeof(Jac<F>), sums[j]);
        return GA_OK;
    };
    return plonk_batch_chunks(count, batch_max, reserve, pass);
}

// what plonk_<curve>.hip instantiates: these five and the four of plonk.hip.h
#define GA_INSTANTIATE_PLONK(C)                                                                                                          \
    template int plonk_domain_quotient<C>(Domain*, Domain*, const PlonkQuotientArgs&, void*);                                            \
    template int plonk_domain_fixed_create<C>(Domain*, Domain*, const PlonkQuotientArgs&, PlonkFixed**);                                 \
    template int fr_vec_batch_inverse<C>(Ctx*, void*, uint64_t, bool);                                                                   \
    template int fr_vec_lincomb<C>(Ctx*, uint64_t, int, const void* const*, const void*, void*, bool);                                   \
    template int plonk_domain_build_z_batch<C>(Domain*, const void*, const void*, const void*, const int64_t*, const void*, const void*, \
                                               uint32_t, PlonkBatchKnobs, bool, void*);                                                  \
    template int plonk_domain_quotient_pinned_batch<C>(PlonkFixed*, const PlonkQuotientArgs*, uint32_t, PlonkBatchKnobs, void*);         \
    template int kzg_domain_divide_batch<C>(Ctx*, const void* const*, uint64_t, uint32_t, const void*, void*, uint64_t, void*, uint64_t, \
                                            std::vector<uint32_t>*);                                                                     \
    template int kzg_domain_divide<C>(Ctx*, const void*, uint64_t, const void*, void*, bool, uint64_t);                                  \
    template int kzg_open_run<C>(MsmTable*, const void* const*, size_t, uint32_t, unsigned, const void*, void*, void*, PlonkBatchKnobs);

}  // namespace ga

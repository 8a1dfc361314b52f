// The three PLONK-specific calls for MANY proofs of one circuit per device pass: the grand product (ga_plonk_build_z_batch), the
// quotient over a pinned key (ga_plonk_quotient_pinned_batch) and the division of kzg.Open (ga_kzg_open_batch).  A loop over proofs
// of the single calls of plonk.hip.h is a chain of launches that one small proof (2^10 .. 2^16 gates) leaves almost empty, each with
// host-built power tables, synchronous uploads and a closing synchronisation.  Here the proof is the grid's y dimension (or a
// segment of a flat index), the per-proof challenges come from a device array uploaded once per pass, every power table is built on
// the device, the scans are segmented per proof, and a pass of up to PLONK_BATCH_LIMIT proofs of the grand product or the quotient ends
// in ONE synchronisation (an opening pass has none of its own beside those of its table MSM).
// Every stored field element is fully reduced, so row j of every output equals the single call's result on item j bit for bit
// whatever the association order of the scans.
#pragma once
#include "plonk.hip.h"

namespace ga {

// ---- power tables on the device ------------------------------------------------------------------------------------------------
// Table t (grid row y) of `bases` = (base_t, c0_t): the two-level table plonk_point reads, lo[k] = c0 * base^k for k < 2^lo_bits and
// hi[k] = base^(k << lo_bits) for k < nhi, (2^lo_bits + nhi) elements per table (the layout of ntt_pow_table_host).  One thread per
// entry, square-and-multiply on the entry's exponent: at most 2 * 64 products, no dependence between threads.
template <class FrP>
__global__ void fr_pow_tables_kernel(const uint32_t* __restrict__ bases, uint32_t* __restrict__ tabs, int lo_bits, uint64_t nhi) {
    const uint64_t nlo = 1ull << lo_bits;
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nlo + nhi) return;
    const uint32_t* b = bases + (size_t)blockIdx.y * 16;
    Fe<FrP> a = load_fe<FrP>(b);
    const bool low = k < nlo;
    uint64_t e = low ? k : (k - nlo) << lo_bits;
    Fe<FrP> r = low ? load_fe<FrP>(b + 8) : fe_one<FrP>();
    while (e) {
        if (e & 1) r = mul_val(r, a);
        a = mul_val(a, a);
        e >>= 1;
    }
    store_fe(tabs + ((size_t)blockIdx.y * (nlo + nhi) + k) * 8, r);
}

// `ntab` tables that cover exponents below n, from host pairs (base, c0), into scratch `key` (pairs first, then the tables): one small
// upload from `stage` -- which the caller keeps alive until its synchronisation -- and one launch.
template <class FrP>
struct PowTables {
    uint32_t *bases = nullptr, *tabs = nullptr;   // [ntab] (base, c0), [ntab] tables
    uint64_t words = 0;                           // per table
    uint32_t* lo(uint64_t t) const { return tabs + t * words; }
    uint32_t* hi(uint64_t t) const { return tabs + t * words + ((size_t)8 << NTT_POW_LO_BITS); }
    static uint64_t nhi_of(uint64_t n) { return n ? ((n - 1) >> NTT_POW_LO_BITS) + 1 : 1; }
    static size_t bytes(uint64_t ntab, uint64_t n) { return (size_t)ntab * (64 + (((size_t)1 << NTT_POW_LO_BITS) + nhi_of(n)) * 32); }
    int build(Ctx* ctx, const char* key, const std::vector<uint32_t>& stage, uint64_t ntab, uint64_t n) {
        const uint64_t nhi = nhi_of(n), per = (1ull << NTT_POW_LO_BITS) + nhi;
        uint32_t* d;
        GA_CHECK(ctx->scratch_get(key, bytes(ntab, n), (void**)&d));
        GA_HIP_CHECK(hipMemcpyAsync(d, stage.data(), ntab * 64, hipMemcpyHostToDevice, ctx->stream));
        bases = d;
        tabs = d + ntab * 16;
        words = per * 8;
        hipLaunchKernelGGL((fr_pow_tables_kernel<FrP>), dim3((unsigned)((per + 255) / 256), (unsigned)ntab), dim3(256), 0, ctx->stream, d, tabs,
                           NTT_POW_LO_BITS, nhi);
        GA_KERNEL_CHECK();
        return GA_OK;
    }
};
template <class FrP>
void pow_pair(std::vector<uint32_t>& stage, const Fe<FrP>& base, const Fe<FrP>& c0) {
    stage.insert(stage.end(), base.l, base.l + 8);
    stage.insert(stage.end(), c0.l, c0.l + 8);
}

// threads of fr_batch_inverse_kernel over `total` elements: each pays one field inversion (~ 400 products) beside three products per
// element, so 16 .. 64 elements per thread; the single call's 64 would leave sixteen proofs of 2^10 on 256 threads
inline uint64_t plonk_inverse_threads(uint64_t total) {
    const uint64_t per = total >= (1ull << 20) ? 64 : total >= (1ull << 17) ? 32 : 16;
    return (total + per - 1) / per;
}

// ---- grand product ---------------------------------------------------------------------------------------------------------------
// plonk_ratio_terms_kernel with the proof in blockIdx.y: L, R, O, num, den are [count][n]; bg[proof] = (beta, gamma); the identity
// tables, the coset shifts and the permutation are the circuit's
template <class FrP>
__global__ void plonk_ratio_terms_batch_kernel(const uint32_t* __restrict__ L, const uint32_t* __restrict__ R, const uint32_t* __restrict__ O,
                                               const int64_t* __restrict__ perm, const uint32_t* __restrict__ w_lo,
                                               const uint32_t* __restrict__ w_hi, int lo_bits, const uint32_t* __restrict__ bg,
                                               const uint32_t* __restrict__ shifts, uint32_t* __restrict__ num, uint32_t* __restrict__ den,
                                               uint64_t n) {
    typedef Fe<FrP> F;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t row = (size_t)blockIdx.y * n * 8;
    const F beta = load_fe<FrP>(bg + (size_t)blockIdx.y * 16), gamma = load_fe<FrP>(bg + (size_t)blockIdx.y * 16 + 8);
    const F shift[3] = {fe_one<FrP>(), load_fe<FrP>(shifts), load_fe<FrP>(shifts + 8)};
    const uint32_t* e[3] = {L + row, R + row, O + row};
    auto idv = [&](uint64_t pos) {   // evaluation of the identity permutation at flat position pos: u^(pos / n) * w^(pos % n)
        uint64_t k = pos / n, j = pos % n;
        F w = plonk_point<FrP>(w_lo, w_hi, lo_bits, j);
        return k == 0 ? w : mul(w, shift[k]);
    };
    F a = fe_one<FrP>(), b = fe_one<FrP>();
    for (int k = 0; k < 3; k++) {
        F v = add(load_fe<FrP>(e[k] + i * 8), gamma);
        a = mul(a, add(v, mul(beta, idv((uint64_t)k * n + i))));
        b = mul(b, add(v, mul(beta, idv((uint64_t)perm[(uint64_t)k * n + i]))));
    }
    store_fe(num + row + i * 8, a);
    store_fe(den + row + i * 8, b);
}

// Segmented exclusive prefix product, z[p][0] = 1, z[p][i] = prod_{t<i} num[p][t] * den_inv[p][t], in the three phases of the single
// call with the segment = the proof: `chunk` divides n (both powers of two, chunk <= n), so a chunk never spans two proofs and a
// proof has cpp = n / chunk chunk products, scanned by one block per proof (blockIdx.y).
template <class FrP>
__global__ void fr_seg_chunk_product_kernel(const uint32_t* __restrict__ num, const uint32_t* __restrict__ den_inv,
                                            uint32_t* __restrict__ chunk_prod, uint64_t total, uint64_t chunk) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t lo = c * chunk;
    if (lo >= total) return;
    Fe<FrP> acc = fe_one<FrP>();
    for (uint64_t i = lo; i < lo + chunk; i++) acc = mul(acc, mul(load_fe<FrP>(num + i * 8), load_fe<FrP>(den_inv + i * 8)));
    store_fe(chunk_prod + c * 8, acc);
}
template <class FrP>
__global__ void __launch_bounds__(256) fr_seg_chunk_scan_kernel(uint32_t* __restrict__ chunk_prod, uint64_t cpp) {
    // fr_chunk_scan_kernel on the cpp chunk products of proof blockIdx.y
    __shared__ uint32_t sh[256 * 8];
    uint32_t* cp = chunk_prod + (size_t)blockIdx.y * cpp * 8;
    const uint32_t tid = threadIdx.x;
    const uint64_t seg = (cpp + 255) / 256;
    const uint64_t lo = (uint64_t)tid * seg < cpp ? (uint64_t)tid * seg : cpp;
    const uint64_t hi = lo + seg < cpp ? lo + seg : cpp;
    Fe<FrP> acc = fe_one<FrP>();
    for (uint64_t c = lo; c < hi; c++) acc = mul_val(acc, load_fe<FrP>(cp + c * 8));
    store_fe(sh + tid * 8, acc);
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {
        Fe<FrP> v = load_fe<FrP>(sh + tid * 8);
        if (tid >= off) v = mul_val(v, load_fe<FrP>(sh + (tid - off) * 8));
        __syncthreads();
        store_fe(sh + tid * 8, v);
        __syncthreads();
    }
    acc = tid ? load_fe<FrP>(sh + (tid - 1) * 8) : fe_one<FrP>();
    for (uint64_t c = lo; c < hi; c++) {
        Fe<FrP> p = load_fe<FrP>(cp + c * 8);
        store_fe(cp + c * 8, acc);
        acc = mul_val(acc, p);
    }
}
template <class FrP>
__global__ void fr_seg_chunk_apply_kernel(const uint32_t* __restrict__ num, const uint32_t* __restrict__ den_inv,
                                          const uint32_t* __restrict__ chunk_prefix, uint32_t* __restrict__ z, uint64_t total, uint64_t chunk) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t lo = c * chunk;
    if (lo >= total) return;
    Fe<FrP> acc = load_fe<FrP>(chunk_prefix + c * 8);
    for (uint64_t i = lo; i < lo + chunk; i++) {
        store_fe(z + i * 8, acc);
        acc = mul(acc, mul(load_fe<FrP>(num + i * 8), load_fe<FrP>(den_inv + i * 8)));
    }
}

// iop.BuildRatioCopyConstraint for `count` proofs of one circuit: L, R, O, z_out = [count][n], betas / gammas = count host elements
template <class FrP>
int plonk_build_z_batch(Domain* d0, const void* L, const void* R, const void* O, const int64_t* perm, const void* betas, const void* gammas,
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
            set_error("ga_plonk_build_z_batch: %u entries of the device-resident permutation are outside [0, 3n)", bad);
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
            hipLaunchKernelGGL((plonk_ratio_terms_batch_kernel<FrP>), dim3((unsigned)((n + 255) / 256), cnt), dim3(256), 0, st, dl, dr, dO,
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
            hipLaunchKernelGGL((fr_seg_chunk_product_kernel<FrP>), dim3(cb), dim3(64), 0, st, num, den, cp, total, chunk);
            hipLaunchKernelGGL((fr_seg_chunk_scan_kernel<FrP>), dim3(1, cnt), dim3(256), 0, st, cp, n / chunk);
            hipLaunchKernelGGL((fr_seg_chunk_apply_kernel<FrP>), dim3(cb), dim3(64), 0, st, num, den, cp, dz, total, chunk);
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
// the constraint kernels with the proof in blockIdx.y: proof j reads its constants from K[j], its own polynomials (the ids of
// P.proofs) `stride` words after proof 0's, and writes block `block` of its own h; the pinned evaluations, 1/(x - 1) and the coset's
// points are the key's.  The expression is the single kernel's (plonk_constraints29_at / plonk_constraints_at).
struct PlonkBatchPtrs {
    PlonkPtrs P;       // proof 0
    uint64_t proofs;   // bit id: a per-proof polynomial
    uint64_t stride;   // words from a proof's polynomial to the next proof's
};
template <class FrP, bool LAZY>
__global__ void __launch_bounds__(128)
plonk_constraints_batch_kernel(PlonkBatchPtrs B, const PlonkConsts* __restrict__ K, const uint32_t* __restrict__ x_lo,
                               const uint32_t* __restrict__ x_hi, int lo_bits, const uint32_t* __restrict__ inv_xm1,
                               uint32_t* __restrict__ out, uint64_t out_stride, uint64_t n, int logn) {
    uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint64_t proof = blockIdx.y;
    if constexpr (LAZY)
        plonk_constraints29_at<FrP>(B.P, B.proofs, proof * B.stride, K[proof], x_lo, x_hi, lo_bits, inv_xm1, out + proof * out_stride, n, logn, j);
    else
        plonk_constraints_at<FrP>(B.P, B.proofs, proof * B.stride, K[proof], x_lo, x_hi, lo_bits, inv_xm1, out + proof * out_stride, n, logn, j);
}

// out[v][bitrev(i)] = in[v][i] for the vectors v = blockIdx.y
template <class FrP>
__global__ void fr_bitrev_copy_batch_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ in, uint64_t n, int logn) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t row = (size_t)blockIdx.y * n * 8;
    store_fe(out + row + bitrev64(i, logn) * 8, load_fe<FrP>(in + row + i * 8));
}

// args[0 .. count): the per-proof polynomials of `count` proofs (one nb_bsb, one lagrange_mask, one on_device); h_out = [count][rho * n]
template <class FrP>
int plonk_quotient_pinned_batch(PlonkFixed* fx, const PlonkQuotientArgs* args, uint32_t count, PlonkBatchKnobs knobs, void* h_out) {
    typedef Fe<FrP> F;
    Domain *d0 = fx->d0, *d1 = fx->d1;
    Ctx* ctx = d0->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t n = d0->n;
    const PlonkQuotientArgs& A0 = args[0];
    if (n < 2 || d1->n < n || d1->n % n != 0 || A0.nb_bsb > (uint32_t)PLONK_MAX_BSB || d1->ctx != ctx) {
        set_error("plonk: need n >= 2, |domain1| a multiple of |domain0|, at most %d BSB22 gates", PLONK_MAX_BSB);
        return GA_ERR_INVALID;
    }
    if (fx->nb_bsb != A0.nb_bsb) {
        set_error("plonk quotient: the pinned key was built for %u BSB22 gates", fx->nb_bsb);
        return GA_ERR_INVALID;
    }
    const uint64_t rho = d1->n / n;
    const int np = PLONK_NB_FIXED + 2 * (int)A0.nb_bsb, logrho = ilog2_u64(rho);
    // the per-proof ids, those given as evaluations first: slot s holds [cnt][n], so the inverse transforms are the first nlag * cnt
    // vectors of the canonical buffer and the bit-reversing copies the rest
    std::vector<int> ids;
    for (int lag = 1; lag >= 0; lag--)
        for (int p : plonk_ids(np, false))
            if ((int)((A0.lagrange_mask >> p) & 1) == lag) ids.push_back(p);
    const uint64_t k = ids.size();
    uint64_t nlag = 0;
    for (int p : ids) nlag += (A0.lagrange_mask >> p) & 1;
    // the cosets: shift g * w1^i, coset^n - 1, the twiddle table, and (on the device) the table of the points coset * w0^j
    std::vector<F> cexp(rho);
    std::vector<PlonkConsts> Kc(rho);   // per coset: what does not depend on the proof (plonk_coset_consts: one inversion per coset)
    std::vector<const uint32_t*> coset_tw(rho);
    std::vector<uint32_t> xstage;
    {
        F coset = fe_one<FrP>();
        for (uint64_t i = 0; i < rho; i++) {
            coset = mul(coset, i == 0 ? fe_const<FrP>(FrP::GEN) : plonk_ld<FrP>(d1->w));   // shifters, prove.go:936-941,998
            cexp[i] = sub(plonk_host_pow<FrP>(coset, n), fe_one<FrP>());
            memset(&Kc[i], 0, sizeof(PlonkConsts));
            plonk_coset_consts<FrP>(Kc[i], d0, cexp[i]);
            GA_CHECK(ntt_coset_table<FrP>(d0, coset, &coset_tw[i]));
            pow_pair<FrP>(xstage, plonk_ld<FrP>(d0->w), coset);
        }
    }
    PowTables<FrP> xt;
    GA_CHECK(xt.build(ctx, "plonk_qb_xtab", xstage, rho, n));
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
        // the constants of every (coset, proof), as PlonkRun::begin_coset + proof_consts make them
        hK.resize((size_t)rho * cnt);
        for (uint64_t i = 0; i < rho; i++)
            for (uint32_t j = 0; j < cnt; j++) {
                hK[i * cnt + j] = Kc[i];
                plonk_proof_consts<FrP>(hK[i * cnt + j], A[j], cexp[i]);
            }
        GA_HIP_CHECK(hipMemcpyAsync(dK, hK.data(), hK.size() * sizeof(PlonkConsts), hipMemcpyHostToDevice, st));
        // to canonical coefficients in bit-reversed order: one inverse DIF over the evaluation vectors (p.ToCanonical, prove.go:1036),
        // one bit-reversing copy over the coefficient vectors
        if (nlag) GA_CHECK(ntt_run<FrP>(d0, canon, /*inverse=*/true, /*dit=*/false, scale_none(), scale_const(d0->ninv), nullptr, nullptr, nlag * cnt));
        if (k > nlag) {
            StageTimer tm(ctx, "plonk_qb_bitrev");
            hipLaunchKernelGGL((fr_bitrev_copy_batch_kernel<FrP>), dim3((unsigned)((n + 255) / 256), (unsigned)((k - nlag) * cnt)), dim3(256), 0, st,
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
            GA_CHECK(ntt_run<FrP>(d0, work, /*inverse=*/false, /*dit=*/true, scale_none(), scale_none(), canon, coset_tw[i], k * cnt));
            for (int p : plonk_ids(np, true)) B.P.p[p] = fx->evals_of(i, p);
            uint64_t block = 0;   // bitrev_N(rho*j + i) = bitrev_rho(i)*n + bitrev_n(j)
            for (int b = 0; b < logrho; b++) block |= ((i >> b) & 1) << (logrho - 1 - b);
            StageTimer tm(ctx, "plonk_qb_constraints");
            constexpr bool LAZY = Radix<FrP>::NL * Radix<FrP>::L - FrP::BITS >= 7;   // BN254: lazy representation; BLS12-381: packed
            hipLaunchKernelGGL((plonk_constraints_batch_kernel<FrP, LAZY>), dim3((unsigned)((n + 127) / 128), cnt), dim3(128), 0, st, B,
                               (const PlonkConsts*)(dK + i * cnt), xt.lo(i), xt.hi(i), NTT_POW_LO_BITS, fx->inv_xm1_of(i), cres + block * n * 8,
                               d1->n * 8, n, d0->logn);
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
    const int rc = plonk_batch_chunks(count, knobs.batch_max, reserve, pass);
    if (rc != GA_OK) hipStreamSynchronize(st);   // the staging vectors above die at return: no copy from them may still be queued
    return rc;
}

// ---- kzg.Open's division for a batch ------------------------------------------------------------------------------------------------
// (p_j(X) - p_j(z_j)) / (X - z_j) as in kzg_divide_by_linear: scaling by z_j^i, suffix sum, scaling by z_j^-(k+1); item j is grid row
// j of the element-wise kernels and a segment of cpp = ceil(n / chunk) chunks of the scan (n is not a power of two: n + 2, n + 3)
struct KzgBatchPtrs {
    const uint32_t* p[PLONK_BATCH_LIMIT];
};
template <class FrP>
__global__ void kzg_scale_batch_kernel(KzgBatchPtrs in, uint32_t* __restrict__ t, const uint32_t* __restrict__ tabs, uint64_t tab_words,
                                       int lo_bits, uint64_t n) {
    // t[j][i] = p_j[i] * z_j^i (table 2j)
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* lo = tabs + (size_t)(2 * blockIdx.y) * tab_words;
    store_fe(t + ((size_t)blockIdx.y * n + i) * 8,
             mul(load_fe<FrP>(in.p[blockIdx.y] + i * 8), plonk_point<FrP>(lo, lo + ((size_t)8 << lo_bits), lo_bits, i)));
}
template <class FrP>
__global__ void fr_seg_chunk_sum_kernel(const uint32_t* __restrict__ t, uint32_t* __restrict__ chunk_sum, uint64_t n, uint64_t chunk,
                                        uint64_t cpp, uint64_t nchunks) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchunks) return;
    const uint64_t row = (c / cpp) * n, lo = (c % cpp) * chunk;
    const uint64_t hi = lo + chunk < n ? lo + chunk : n;
    Fe<FrP> acc = fe_zero<FrP>();
    for (uint64_t i = lo; i < hi; i++) acc = add(acc, load_fe<FrP>(t + (row + i) * 8));
    store_fe(chunk_sum + c * 8, acc);
}
template <class FrP>
__global__ void __launch_bounds__(256) fr_seg_chunk_suffix_scan_kernel(uint32_t* __restrict__ chunk_sum, uint64_t cpp) {
    // fr_chunk_suffix_scan_kernel on the cpp chunk sums of item blockIdx.y
    __shared__ uint32_t sh[256 * 8];
    uint32_t* cs = chunk_sum + (size_t)blockIdx.y * cpp * 8;
    const uint32_t tid = threadIdx.x;
    const uint64_t seg = (cpp + 255) / 256;
    const uint64_t lo = (uint64_t)tid * seg < cpp ? (uint64_t)tid * seg : cpp;
    const uint64_t hi = lo + seg < cpp ? lo + seg : cpp;
    Fe<FrP> acc = fe_zero<FrP>();
    for (uint64_t c = lo; c < hi; c++) acc = add(acc, load_fe<FrP>(cs + c * 8));
    store_fe(sh + tid * 8, acc);
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {   // inclusive suffix scan over the 256 segment sums
        Fe<FrP> v = load_fe<FrP>(sh + tid * 8);
        if (tid + off < 256) v = add(v, load_fe<FrP>(sh + (tid + off) * 8));
        __syncthreads();
        store_fe(sh + tid * 8, v);
        __syncthreads();
    }
    acc = tid + 1 < 256 ? load_fe<FrP>(sh + (tid + 1) * 8) : fe_zero<FrP>();   // everything after this thread's segment
    for (uint64_t c = hi; c-- > lo;) {
        Fe<FrP> v = load_fe<FrP>(cs + c * 8);
        store_fe(cs + c * 8, acc);
        acc = add(acc, v);
    }
}
template <class FrP>
__global__ void fr_seg_chunk_suffix_apply_kernel(uint32_t* __restrict__ t, const uint32_t* __restrict__ chunk_after, uint64_t n, uint64_t chunk,
                                                 uint64_t cpp, uint64_t nchunks) {
    // t[j][i] <- sum_{i' >= i} t[j][i']  (inclusive suffix sum per item)
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchunks) return;
    const uint64_t row = (c / cpp) * n, lo = (c % cpp) * chunk;
    const uint64_t hi = lo + chunk < n ? lo + chunk : n;
    Fe<FrP> acc = load_fe<FrP>(chunk_after + c * 8);
    for (uint64_t i = hi; i-- > lo;) {
        acc = add(acc, load_fe<FrP>(t + (row + i) * 8));
        store_fe(t + (row + i) * 8, acc);
    }
}
template <class FrP>
__global__ void kzg_quotient_batch_kernel(KzgBatchPtrs in, const uint32_t* __restrict__ t, const uint32_t* __restrict__ bases,
                                          const uint32_t* __restrict__ tabs, uint64_t tab_words, int lo_bits, uint64_t n,
                                          uint32_t* __restrict__ quot, uint64_t quot_stride, uint32_t* __restrict__ values) {
    // q_j[i] = S_j[i + 1] * z_j^-(i + 1) (table 2j + 1), or p_j[i + 1] where z_j = 0; values[j] = S_j[0] = p_j(z_j)
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t* tj = t + (size_t)blockIdx.y * n * 8;
    if (i == 0) store_fe(values + (size_t)blockIdx.y * 8, load_fe<FrP>(tj));
    if (i + 1 >= n) return;
    Fe<FrP> q;
    if (is_zero(load_fe<FrP>(bases + (size_t)(2 * blockIdx.y) * 16))) {
        q = load_fe<FrP>(in.p[blockIdx.y] + (i + 1) * 8);
    } else {
        const uint32_t* lo = tabs + (size_t)(2 * blockIdx.y + 1) * tab_words;
        q = mul(load_fe<FrP>(tj + (i + 1) * 8), plonk_point<FrP>(lo, lo + ((size_t)8 << lo_bits), lo_bits, i + 1));
    }
    store_fe(quot + (size_t)blockIdx.y * quot_stride * 8 + i * 8, q);
}

template <class FrP>
int kzg_divide_by_linear_batch(Ctx* ctx, const void* const* d_polys, uint64_t n, uint32_t count, const void* points, uint32_t* d_quot,
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
    // `stage`, which lives until the caller's MSM has returned (that MSM synchronises the stream)
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
    hipLaunchKernelGGL((kzg_scale_batch_kernel<FrP>), dim3(blocks, count), dim3(256), 0, st, in, t, pt.tabs, pt.words, NTT_POW_LO_BITS, n);
    hipLaunchKernelGGL((fr_seg_chunk_sum_kernel<FrP>), dim3(cb), dim3(64), 0, st, t, cs, n, chunk, cpp, nchunks);
    hipLaunchKernelGGL((fr_seg_chunk_suffix_scan_kernel<FrP>), dim3(1, count), dim3(256), 0, st, cs, cpp);
    hipLaunchKernelGGL((fr_seg_chunk_suffix_apply_kernel<FrP>), dim3(cb), dim3(64), 0, st, t, cs, n, chunk, cpp, nchunks);
    hipLaunchKernelGGL((kzg_quotient_batch_kernel<FrP>), dim3(blocks, count), dim3(256), 0, st, in, (const uint32_t*)t,
                       (const uint32_t*)pt.bases, (const uint32_t*)pt.tabs, pt.words, NTT_POW_LO_BITS, n, d_quot,
                       quot_stride, d_values);
    GA_KERNEL_CHECK();
    return GA_OK;
}

}  // namespace ga

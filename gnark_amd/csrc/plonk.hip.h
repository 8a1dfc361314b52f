// PLONK quotient on the device: computeNumerator + divideByZH of backend/plonk/bn254/prove.go:841-1123,1287-1350
// (SURVEY 8f row 4), and the grand-product polynomial of iop.BuildRatioCopyConstraint (call site prove.go:645-655).
//
// The reference keeps 13+2k polynomials of size n on the CPU and, for each of the rho = |domain1|/n cosets
// coset_i = g*w1^i, converts every polynomial back to canonical form, rescales it and runs a forward FFT (two FFTs per
// polynomial and coset, prove.go:1033-1058: "we do **a lot** of FFT here").  Here the canonical coefficients stay resident
// in HBM in bit-reversed order (one inverse DIF per polynomial, once), each coset costs ONE out-of-place coset DIT per
// polynomial over a twiddle table that carries the coset shift (ntt_coset_table), the pointwise constraint (gate + alpha*ordering +
// alpha^2*(Z-1)*L1, blinding included) is one kernel that also applies divideByZH's 1/(X^n-1) factor and writes the result
// at its bit-reversed slot, and the final inverse coset transform of size rho*n produces h in canonical order.
// 1/(x-1) for L1 comes from a batched Montgomery-trick inversion kernel (the reference's batchInvert, prove.go:1134-1147).
// Field elements are mathematically unique, so the coefficients equal the reference's bit for bit.
//
// The grand product, the quotient over a pinned key and the division of kzg.Open have ONE implementation each, for `count` proofs of
// one circuit per device pass (the drivers of plonk_batch.hip.h; a single proof is count = 1).  The kernels below therefore carry the
// proof in the grid's y dimension (or as a segment of a flat index), read a proof's challenges from a device array, and every power
// table is built on the device.  Every stored field element is fully reduced, so a result does not depend on how a scan associates.
#pragma once
#include "ntt.hip.h"
#include <algorithm>
#include <iterator>
#include <memory>

namespace ga {

// PLONK_MAX_BSB, PLONK_NB_FIXED and PlonkQuotientArgs live in common.hip.h (shared with the ABI translation unit)
enum { PX_L = 0, PX_R, PX_O, PX_Z, PX_QL, PX_QR, PX_QM, PX_QO, PX_QK, PX_S1, PX_S2, PX_S3 };

struct PlonkPtrs {
    const uint32_t* p[PLONK_NB_FIXED + 2 * PLONK_MAX_BSB];   // [12 + 2*i] = Qcp_i, [13 + 2*i] = committed polynomial i
    int nb_bsb;
};

struct PlonkConsts {
    uint32_t alpha[8], beta[8], gamma[8], cs[8], css[8];
    uint32_t bl[2][8], br[2][8], bo[2][8], bz[3][8];   // blinding coefficients already multiplied by (coset^n - 1)
    uint32_t lone[8];      // (coset^n - 1) / n
    uint32_t omega[8];     // generator of the small domain
    uint32_t zh_inv[8];    // 1 / (coset^n - 1): divideByZH's factor for this coset (prove.go:1327-1350)
    // 32 * c mod r of the constants that the lazy constraint kernel multiplies by (plonk_constraints29_at): a product of limb
    // vectors divides by 2^261 where the memory format wants 2^256, so one factor carries the 2^5
    uint32_t sh[11][8];
};
enum { PSH_OMEGA = 0, PSH_BL1, PSH_BR1, PSH_BO1, PSH_BZ2, PSH_BETA, PSH_CS, PSH_CSS, PSH_LONE, PSH_ALPHA, PSH_ZHINV };

template <class FrP>
__device__ __forceinline__ Fe<FrP> plonk_c(const uint32_t* w) {
    Fe<FrP> r;
#pragma unroll
    for (int k = 0; k < 8; k++) r.l[k] = w[k];
    return r;
}

// x_j = coset * w^j from the two power tables (lo: coset*w^k, k < 2^lo_bits; hi: w^(k << lo_bits)), plain Montgomery form
template <class FrP>
__device__ __forceinline__ Fe<FrP> plonk_point(const uint32_t* lo, const uint32_t* hi, int lo_bits, uint64_t j) {
    Fe<FrP> a = load_fe<FrP>(lo + (j & ((1ull << lo_bits) - 1)) * 8);
    uint64_t h = j >> lo_bits;
    return h ? mul(a, load_fe<FrP>(hi + h * 8)) : a;
}

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

template <class FrP>
__global__ void plonk_x_minus_one_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi,
                                         int lo_bits, uint64_t n) {
    uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    store_fe(out + j * 8, sub(plonk_point<FrP>(lo, hi, lo_bits, j), fe_one<FrP>()));
}

// In-place batched inversion (Montgomery's trick; zeros stay zero like fr.BatchInvert).  Thread t owns elements
// t, t+T, t+2T, ... (T = total threads): every access is coalesced across the wave; tmp holds the running products.
template <class FrP>
__global__ void fr_batch_inverse_kernel(uint32_t* __restrict__ v, uint32_t* __restrict__ tmp, uint64_t n) {
    const uint64_t T = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    Fe<FrP> acc = fe_one<FrP>();
    for (uint64_t i = t; i < n; i += T) {
        store_fe(tmp + i * 8, acc);   // product of the (non-zero) elements before i
        Fe<FrP> x = load_fe<FrP>(v + i * 8);
        if (!is_zero(x)) acc = mul(acc, x);
    }
    acc = inv(acc);
    uint64_t last = t + ((n - 1 - t) / T) * T;
    for (uint64_t i = last;; i -= T) {
        Fe<FrP> x = load_fe<FrP>(v + i * 8);
        if (!is_zero(x)) {
            store_fe(v + i * 8, mul(acc, load_fe<FrP>(tmp + i * 8)));
            acc = mul(acc, x);
        }
        if (i == t) break;
    }
}

// threads of fr_batch_inverse_kernel over `total` elements, for every caller: each pays one field inversion (~ 400 products) beside
// three products per element, so 16 .. 64 elements per thread; 64 throughout would leave sixteen proofs of 2^10 on 256 threads
inline uint64_t plonk_inverse_threads(uint64_t total) {
    const uint64_t per = total >= (1ull << 20) ? 64 : total >= (1ull << 17) ? 32 : 16;
    return (total + per - 1) / per;
}

// allConstraints of prove.go:950-981 at point j of the current coset, times 1/(X^n-1) on this coset (divideByZH,
// prove.go:1311-1316), stored where the big inverse DIT expects evaluation rho*j + i: block*n + bitrev_n(j) (prove.go:1073).
// proofs / stride: the polynomials whose id is in the bit set `proofs` are read `stride` words further on (a proof's own polynomials,
// plonk_constraints_kernel below).
template <class FrP>
__device__ __forceinline__ void plonk_constraints_at(const PlonkPtrs& P, uint64_t proofs, uint64_t stride, const PlonkConsts& K,
                                                     const uint32_t* __restrict__ x_lo, const uint32_t* __restrict__ x_hi, int lo_bits,
                                                     const uint32_t* __restrict__ inv_xm1, uint32_t* __restrict__ out_block, uint64_t n, int logn,
                                                     uint64_t j) {
    typedef Fe<FrP> F;
    // ~45 products per point against 14 x 32 B of loads: one shared out-of-line multiply keeps the kernel small
    auto mul = [](const F& u, const F& v) { return mul_val(u, v); };
    auto at = [&](int id, uint64_t idx) { return load_fe<FrP>(P.p[id] + ((proofs >> id) & 1 ? stride : 0) + idx * 8); };
    const F x = plonk_point<FrP>(x_lo, x_hi, lo_bits, j);
    const F xw = mul(x, plonk_c<FrP>(K.omega));   // next point of the coset: ZS is Z shifted by one (prove.go:602,972)
    const F beta = plonk_c<FrP>(K.beta), gamma = plonk_c<FrP>(K.gamma), alpha = plonk_c<FrP>(K.alpha);
    // blinded wires (prove.go:957-973): p + b(x)*(x^n - 1), the factor (coset^n - 1) is folded into the coefficients
    F l = add(at(PX_L, j), add(plonk_c<FrP>(K.bl[0]), mul(plonk_c<FrP>(K.bl[1]), x)));
    F r = add(at(PX_R, j), add(plonk_c<FrP>(K.br[0]), mul(plonk_c<FrP>(K.br[1]), x)));
    F o = add(at(PX_O, j), add(plonk_c<FrP>(K.bo[0]), mul(plonk_c<FrP>(K.bo[1]), x)));
    auto bz = [&](const F& pt) {
        return add(plonk_c<FrP>(K.bz[0]), mul(pt, add(plonk_c<FrP>(K.bz[1]), mul(pt, plonk_c<FrP>(K.bz[2])))));
    };
    F z = add(at(PX_Z, j), bz(x));
    F zs = add(at(PX_Z, j + 1 == n ? 0 : j + 1), bz(xw));
    // gate (prove.go:868-885)
    F gate = add(mul(at(PX_QL, j), l), mul(at(PX_QR, j), r));
    gate = add(gate, mul(mul(at(PX_QM, j), l), r));
    gate = add(gate, mul(at(PX_QO, j), o));
    gate = add(gate, at(PX_QK, j));
    for (int t = 0; t < P.nb_bsb; t++) gate = add(gate, mul(at(PLONK_NB_FIXED + 2 * t, j), at(PLONK_NB_FIXED + 2 * t + 1, j)));
    // ordering (prove.go:898-923)
    F id = mul(x, beta);
    F a = add(add(gamma, l), id);
    F b = add(add(mul(id, plonk_c<FrP>(K.cs)), r), gamma);
    F c = add(add(mul(id, plonk_c<FrP>(K.css)), o), gamma);
    F rr = mul(mul(mul(a, b), c), z);
    a = add(add(mul(at(PX_S1, j), beta), l), gamma);
    b = add(add(mul(at(PX_S2, j), beta), r), gamma);
    c = add(add(mul(at(PX_S3, j), beta), o), gamma);
    F ll = mul(mul(mul(a, b), c), zs);
    F ord = sub(ll, rr);
    // local (prove.go:926-934, 380-385)
    F lone = mul(plonk_c<FrP>(K.lone), load_fe<FrP>(inv_xm1 + j * 8));
    F loc = mul(sub(z, fe_one<FrP>()), lone);
    F res = add(mul(add(mul(loc, alpha), ord), alpha), gate);
    res = mul(res, plonk_c<FrP>(K.zh_inv));
    store_fe(out_block + bitrev64(j, logn) * 8, res);
}

// The same expression in the lazy representation (field29.hip.h) for scalar fields with >= 7 spare bits in nine 29-bit limbs
// (BN254's Fr; BASELINE config 5): values are memory images x * 2^256 held as unreduced limbs -- additions are limb-wise with one carry
// sweep and no modular correction, a product is f29_mul (162 multiply-adds + a shift / mask per column, ~250 instructions inline
// against ~360 + a call for the packed product).  f29_mul divides by 2^261, the memory format by 2^256: a product takes one factor
// times 32 -- a constant as its precomputed image 32 c mod r (PlonkConsts::sh: canonical, so the other factor may be anything below
// 2^261), a variable by a 5-bit limb shift (it must then be below 2^256 = 5.29 r).  Every intermediate's bound: tools/lazy_bounds.py
// check_plonk_constraints (largest value 27 r of the 169 r that fit); one exact reduction at the store.
template <class FrP>
__device__ __forceinline__ F29<FrP> plonk_shl5(const F29<FrP>& a) {   // 32 a for a normalized a < 2^256
    constexpr int L = Radix<FrP>::L, NL = Radix<FrP>::NL;
    constexpr uint32_t MASK = (1u << L) - 1;
    F29<FrP> r;
    r.l[0] = (a.l[0] << 5) & MASK;
#pragma unroll
    for (int i = 1; i < NL - 1; i++) r.l[i] = ((a.l[i] << 5) & MASK) | (a.l[i - 1] >> (L - 5));
    r.l[NL - 1] = (a.l[NL - 1] << 5) | (a.l[NL - 2] >> (L - 5));
    return r;
}
template <class FrP>
__device__ __forceinline__ void plonk_constraints29_at(const PlonkPtrs& P, uint64_t proofs, uint64_t stride, const PlonkConsts& K,
                                                       const uint32_t* __restrict__ x_lo, const uint32_t* __restrict__ x_hi, int lo_bits,
                                                       const uint32_t* __restrict__ inv_xm1, uint32_t* __restrict__ out_block, uint64_t n, int logn,
                                                       uint64_t j) {
    static_assert(Radix<FrP>::NL * Radix<FrP>::L - 32 * FrP::N == 5 && Radix<FrP>::NL * Radix<FrP>::L - FrP::BITS >= 7,
                  "the shift-by-5 products and the bounds of tools/lazy_bounds.py need nine 29-bit limbs over a <= 254-bit modulus");
    typedef F29<FrP> E;
    auto at = [&](int id, uint64_t idx) { return f29_unpack(load_fe<FrP>(P.p[id] + ((proofs >> id) & 1 ? stride : 0) + idx * 8)); };   // canonical
    auto cst = [&](const uint32_t* w) { return f29_unpack(plonk_c<FrP>(w)); };                       // canonical
    auto mulc = [&](int sh_id, const E& v) { return f29_mul(cst(K.sh[sh_id]), v); };                 // constant x anything below 2^261
    auto mulv = [&](const E& small, const E& v) { return f29_mul(plonk_shl5<FrP>(small), v); };      // `small` below 2^256
    E x = f29_unpack(load_fe<FrP>(x_lo + (j & ((1ull << lo_bits) - 1)) * 8));
    if (const uint64_t h = j >> lo_bits) x = mulv(x, f29_unpack(load_fe<FrP>(x_hi + h * 8)));
    const E xw = mulc(PSH_OMEGA, x);   // next point of the coset: ZS is Z shifted by one (prove.go:602,972)
    const E gamma = cst(K.gamma);
    // blinded wires (prove.go:957-973)
    const E l = f29_add(at(PX_L, j), f29_add(cst(K.bl[0]), mulc(PSH_BL1, x)));
    const E r = f29_add(at(PX_R, j), f29_add(cst(K.br[0]), mulc(PSH_BR1, x)));
    const E o = f29_add(at(PX_O, j), f29_add(cst(K.bo[0]), mulc(PSH_BO1, x)));
    auto bz = [&](const E& pt) { return f29_add(cst(K.bz[0]), mulv(pt, f29_add(cst(K.bz[1]), mulc(PSH_BZ2, pt)))); };
    const E z = f29_add(at(PX_Z, j), bz(x));
    const E zs = f29_add(at(PX_Z, j + 1 == n ? 0 : j + 1), bz(xw));
    // gate (prove.go:868-885): the circuit-constant factor is canonical, so it is the one that takes the shift
    E gate = f29_add(mulv(at(PX_QL, j), l), mulv(at(PX_QR, j), r));
    gate = f29_add(gate, mulv(mulv(at(PX_QM, j), l), r));
    gate = f29_add(gate, mulv(at(PX_QO, j), o));
    gate = f29_add(gate, at(PX_QK, j));
    for (int t = 0; t < P.nb_bsb; t++) gate = f29_add(gate, mulv(at(PLONK_NB_FIXED + 2 * t, j), at(PLONK_NB_FIXED + 2 * t + 1, j)));
    // ordering (prove.go:898-923): each three-term factor stays below 2^256, the running product is always the un-shifted operand
    const E id = mulc(PSH_BETA, x);
    E a = f29_add(f29_add(gamma, l), id);
    E b = f29_add(f29_add(mulc(PSH_CS, id), r), gamma);
    E c = f29_add(f29_add(mulc(PSH_CSS, id), o), gamma);
    const E rr = mulv(z, mulv(c, mulv(a, b)));
    a = f29_add(f29_add(mulc(PSH_BETA, at(PX_S1, j)), l), gamma);
    b = f29_add(f29_add(mulc(PSH_BETA, at(PX_S2, j)), r), gamma);
    c = f29_add(f29_add(mulc(PSH_BETA, at(PX_S3, j)), o), gamma);
    const E ll = mulv(zs, mulv(c, mulv(a, b)));
    const E ord = f29_sub<8>(ll, rr);
    // local (prove.go:926-934, 380-385)
    const E lone = mulc(PSH_LONE, f29_unpack(load_fe<FrP>(inv_xm1 + j * 8)));
    const E loc = mulv(lone, f29_sub<2>(z, f29_unpack(fe_one<FrP>())));
    E res = f29_add(mulc(PSH_ALPHA, f29_add(mulc(PSH_ALPHA, loc), ord)), gate);
    res = mulc(PSH_ZHINV, res);
    store_fe(out_block + bitrev64(j, logn) * 8, f29_pack_canonical(f29_reduce_3p(res)));
}

// The constraint launch, with the proof in blockIdx.y: proof j reads its constants from K[j], its own polynomials (the ids of
// B.proofs) `stride` words after proof 0's, and writes its block of its own h, out_stride words after proof 0's; whatever else it
// reads (pinned evaluations, 1/(x - 1), the coset's points) is shared.  LAZY: the expression on unreduced limbs, BN254; BLS12-381's
// 255-bit Fr leaves 6 spare bits and stays packed.
template <class FrP>
constexpr bool PLONK_LAZY = Radix<FrP>::NL * Radix<FrP>::L - FrP::BITS >= 7;
struct PlonkBatchPtrs {
    PlonkPtrs P;       // proof 0
    uint64_t proofs;   // bit id: a per-proof polynomial
    uint64_t stride;   // words from a proof's polynomial to the next proof's
};
template <class FrP, bool LAZY>
__global__ void __launch_bounds__(128)
plonk_constraints_kernel(PlonkBatchPtrs B, const PlonkConsts* __restrict__ K, const uint32_t* __restrict__ x_lo,
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
__global__ void fr_bitrev_copy_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ in, uint64_t n, int logn) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t row = (size_t)blockIdx.y * n * 8;
    store_fe(out + row + bitrev64(i, logn) * 8, load_fe<FrP>(in + row + i * 8));
}

// ---- grand product (iop.BuildRatioCopyConstraint) --------------------------------------------------------------------
// ratio[i] = prod_k (e_k[i] + beta*id_k(i) + gamma) and its denominator prod_k (e_k[i] + beta*id(perm[k*n+i]) + gamma)
// for the proof blockIdx.y: L, R, O, num, den are [count][n]; bg[proof] = (beta, gamma); the identity tables, the coset shifts and
// the permutation are the circuit's
template <class FrP>
__global__ void plonk_ratio_terms_kernel(const uint32_t* __restrict__ L, const uint32_t* __restrict__ R, const uint32_t* __restrict__ O,
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

// Segmented exclusive prefix product, z[p][0] = 1, z[p][i] = prod_{t<i} num[p][t] * den_inv[p][t], in three phases -- per-chunk
// products, a scan of the chunk products, a per-chunk rescan with the carried-in prefix -- with the segment = the proof: `chunk`
// divides n (both powers of two, chunk <= n), so a chunk never spans two proofs and a proof has cpp = n / chunk chunk products,
// scanned by one block per proof (blockIdx.y).
template <class FrP>
__global__ void fr_chunk_product_kernel(const uint32_t* __restrict__ num, const uint32_t* __restrict__ den_inv,
                                        uint32_t* __restrict__ chunk_prod, uint64_t total, uint64_t chunk) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t lo = c * chunk;
    if (lo >= total) return;
    Fe<FrP> acc = fe_one<FrP>();
    for (uint64_t i = lo; i < lo + chunk; i++) acc = mul(acc, mul(load_fe<FrP>(num + i * 8), load_fe<FrP>(den_inv + i * 8)));
    store_fe(chunk_prod + c * 8, acc);
}
template <class FrP>
__global__ void __launch_bounds__(256) fr_chunk_scan_kernel(uint32_t* __restrict__ chunk_prod, uint64_t cpp) {
    // the cpp chunk products of proof blockIdx.y: each thread multiplies a contiguous segment of them, the 256 segment products are
    // scanned in LDS (Hillis-Steele, 8 steps), then every thread rewrites its segment as exclusive prefixes
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
__global__ void fr_chunk_apply_kernel(const uint32_t* __restrict__ num, const uint32_t* __restrict__ den_inv,
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

// ---- kzg.Open: p(z) and the coefficients of (p(X) - p(z)) / (X - z) -----------------------------------------------------
// gnark-crypto's dividePolyByXminusA is a sequential Horner recurrence q_{k-1} = p_k + z*q_k (call sites
// backend/plonk/bn254/prove.go:681,788,827).  Unrolled, q_k = z^-(k+1) * sum_{j>k} p_j z^j: an element-wise scaling by z^j, a
// suffix SUM (field additions only, three-phase scan) and an element-wise scaling by z^-(k+1); p(z) is the total sum.  Item j is grid
// row j of the element-wise kernels and a segment of cpp = ceil(n / chunk) chunks of the scan (n is not a power of two: n + 2, n + 3)
struct KzgBatchPtrs {
    const uint32_t* p[PLONK_BATCH_LIMIT];
};
template <class FrP>
__global__ void kzg_scale_kernel(KzgBatchPtrs in, uint32_t* __restrict__ t, const uint32_t* __restrict__ tabs, uint64_t tab_words,
                                 int lo_bits, uint64_t n) {
    // t[j][i] = p_j[i] * z_j^i (table 2j)
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* lo = tabs + (size_t)(2 * blockIdx.y) * tab_words;
    store_fe(t + ((size_t)blockIdx.y * n + i) * 8,
             mul(load_fe<FrP>(in.p[blockIdx.y] + i * 8), plonk_point<FrP>(lo, lo + ((size_t)8 << lo_bits), lo_bits, i)));
}
template <class FrP>
__global__ void fr_chunk_sum_kernel(const uint32_t* __restrict__ t, uint32_t* __restrict__ chunk_sum, uint64_t n, uint64_t chunk,
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
__global__ void __launch_bounds__(256) fr_chunk_suffix_scan_kernel(uint32_t* __restrict__ chunk_sum, uint64_t cpp) {
    // chunk_sum[c] <- sum of the chunks AFTER c (exclusive suffix sum) over the cpp chunk sums of item blockIdx.y; segment per thread + LDS scan
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
__global__ void fr_chunk_suffix_apply_kernel(uint32_t* __restrict__ t, const uint32_t* __restrict__ chunk_after, uint64_t n, uint64_t chunk,
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
__global__ void kzg_quotient_kernel(KzgBatchPtrs in, const uint32_t* __restrict__ t, const uint32_t* __restrict__ bases,
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

// ---- host side -----------------------------------------------------------------------------------------------------

template <class FrP>
Fe<FrP> plonk_host_pow(Fe<FrP> a, uint64_t e) {
    Fe<FrP> r = fe_one<FrP>();
    while (e) {
        if (e & 1) r = mul(r, a);
        a = sqr(a);
        e >>= 1;
    }
    return r;
}

// element k of a host array of field elements (Montgomery images) / its words into a kernel argument
template <class FrP>
Fe<FrP> plonk_ld(const void* p, int k = 0) {
    Fe<FrP> f;
    memcpy(f.l, (const char*)p + 32 * k, 32);
    return f;
}
template <class FrP>
void plonk_put(uint32_t* dst, const Fe<FrP>& v) {
    memcpy(dst, v.l, 32);
}

// The constants of the constraint kernel, in two steps: what depends on the coset alone -- cexp = coset^n - 1 (prove.go:999-1000) --, then a proof's challenges, its blinding
// coefficients times cexp, and the images sh[] = 32 c mod r of the constants the lazy kernel multiplies by
template <class FrP>
void plonk_coset_consts(PlonkConsts& K, const Domain* d0, const Fe<FrP>& cexp) {
    const Fe<FrP> g = fe_const<FrP>(FrP::GEN);
    plonk_put(K.cs, g);   // prove.go:891-893
    plonk_put(K.css, sqr(g));
    memcpy(K.omega, d0->w, 32);
    plonk_put(K.lone, mul(cexp, plonk_ld<FrP>(d0->ninv_mont)));
    plonk_put(K.zh_inv, inv(cexp));
}
template <class FrP>
void plonk_proof_consts(PlonkConsts& K, const PlonkQuotientArgs& A, const Fe<FrP>& cexp) {
    typedef Fe<FrP> F;
    plonk_put(K.alpha, plonk_ld<FrP>(A.alpha));
    plonk_put(K.beta, plonk_ld<FrP>(A.beta));
    plonk_put(K.gamma, plonk_ld<FrP>(A.gamma));
    for (int k = 0; k < 2; k++) {
        plonk_put(K.bl[k], mul(plonk_ld<FrP>(A.bl, k), cexp));
        plonk_put(K.br[k], mul(plonk_ld<FrP>(A.br, k), cexp));
        plonk_put(K.bo[k], mul(plonk_ld<FrP>(A.bo, k), cexp));
    }
    for (int k = 0; k < 3; k++) plonk_put(K.bz[k], mul(plonk_ld<FrP>(A.bz, k), cexp));
    const uint32_t* src[11] = {K.omega, K.bl[1], K.br[1], K.bo[1], K.bz[2], K.beta, K.cs, K.css, K.lone, K.alpha, K.zh_inv};   // (index = PSH_*)
    for (int q = 0; q < 11; q++) {   // 32 c mod r: five modular doublings each
        F v = plonk_ld<FrP>(src[q]);
        for (int k = 0; k < 5; k++) v = add(v, v);
        plonk_put(K.sh[q], v);
    }
}

// Circuit-constant part of the quotient, pinned in HBM (the "huge memory footprint" precomputation prove.go:1030-1034 decides
// against on a CPU): the evaluations of Ql, Qr, Qm, Qo, S1, S2, S3 and every Qcp on each of the rho cosets, and 1/(x-1) on
// each coset -- (7 + k + 1) * rho * n * 32 B, 4.3 GB at n = 2^22.  Per proof only L, R, O, Z, Qk and the BSB22 commitment
// polynomials are transformed: 6 + 4*6 + 1 transforms instead of 12 + 4*12 + 1.
struct PlonkFixed {
    Domain *d0 = nullptr, *d1 = nullptr;
    uint32_t nb_bsb = 0;
    int nslots = 0;
    int slot[PLONK_NB_FIXED + 2 * PLONK_MAX_BSB];   // -1: per-proof polynomial; else index into evals
    uint32_t* evals = nullptr;     // [rho][nslots][n] fr
    uint32_t* inv_xm1 = nullptr;   // [rho][n] fr
    uint32_t* evals_of(uint64_t coset, int p) const { return evals + ((size_t)(coset * nslots + slot[p])) * d0->n * 8; }
    uint32_t* inv_xm1_of(uint64_t coset) const { return inv_xm1 + (size_t)coset * d0->n * 8; }
};
inline void plonk_fixed_destroy(PlonkFixed* fx) {
    if (!fx) return;
    hipFree(fx->evals);
    hipFree(fx->inv_xm1);
    delete fx;
}
inline bool plonk_is_fixed(int p) {
    if (p >= PLONK_NB_FIXED) return ((p - PLONK_NB_FIXED) & 1) == 0;               // Qcp_i fixed, Pi2_i per proof
    return p == PX_QL || p == PX_QR || p == PX_QM || p == PX_QO || p == PX_S1 || p == PX_S2 || p == PX_S3;
}
// the ids below np that are (not) circuit constants
inline std::vector<int> plonk_ids(int np, bool fixed) {
    std::vector<int> ids;
    for (int p = 0; p < np; p++)
        if (plonk_is_fixed(p) == fixed) ids.push_back(p);
    return ids;
}

// What every quotient driver needs of the rho cosets g * w1^i of the big domain (shifters, prove.go:936-941,998), made once per call:
// coset^n - 1 (prove.go:999-1000), the constants that depend on the coset alone (one inversion per coset), the twiddle table that
// carries the shift -- kept per domain and coset, so a forward transform scales nothing (prove.go:1033-1058) -- and, on the device,
// the tables of the points coset * w0^j: one small upload out of `stage` and one launch for all cosets.  The owner keeps this object
// alive until it has synchronised.
template <class FrP>
struct PlonkCosets {
    uint64_t rho = 0;
    std::vector<Fe<FrP>> cexp;
    std::vector<PlonkConsts> K;
    std::vector<const uint32_t*> tw;
    std::vector<uint32_t> stage;
    PowTables<FrP> x;

    int build(Domain* d0, Domain* d1, uint32_t nb_bsb) {
        const uint64_t n = d0->n;
        if (n < 2 || d1->n < n || d1->n % n != 0 || nb_bsb > (uint32_t)PLONK_MAX_BSB || d1->ctx != d0->ctx) {
            set_error("plonk: need n >= 2, |domain1| a multiple of |domain0|, at most %d BSB22 gates", PLONK_MAX_BSB);
            return GA_ERR_INVALID;
        }
        rho = d1->n / n;
        cexp.resize(rho), K.resize(rho), tw.resize(rho);
        Fe<FrP> coset = fe_one<FrP>();
        for (uint64_t i = 0; i < rho; i++) {
            coset = mul(coset, i == 0 ? fe_const<FrP>(FrP::GEN) : plonk_ld<FrP>(d1->w));
            cexp[i] = sub(plonk_host_pow<FrP>(coset, n), fe_one<FrP>());
            memset(&K[i], 0, sizeof(PlonkConsts));
            plonk_coset_consts<FrP>(K[i], d0, cexp[i]);
            GA_CHECK(ntt_coset_table<FrP>(d0, coset, &tw[i]));
            pow_pair<FrP>(stage, plonk_ld<FrP>(d0->w), coset);
        }
        return x.build(d0->ctx, "plonk_qb_xtab", stage, rho, n);
    }
    // where the constraints of coset i go: bitrev_N(rho*j + i) = bitrev_rho(i)*n + bitrev_n(j)
    uint64_t block(uint64_t i) const {
        const int logrho = ilog2_u64(rho);
        uint64_t b = 0;
        for (int k = 0; k < logrho; k++) b |= ((i >> k) & 1) << (logrho - 1 - k);
        return b;
    }
};

// One call of ga_plonk_quotient (every polynomial per call) or ga_plonk_pk_create: the checked shape, the scratch buffers and the
// stages as members.  A driver calls begin once, to_canonical per polynomial it owns, proof_consts if it evaluates constraints, then
// per coset the stages it needs.  (The quotient over a pinned key is plonk_quotient_pinned of plonk_batch.hip.h.)
template <class FrP>
struct PlonkRun {
    Ctx* ctx = nullptr;
    Domain *d0, *d1;
    hipStream_t st;
    uint64_t n, rho;
    int np;
    unsigned blocks;                               // of 256 threads over n
    uint32_t *canon, *work, *invb, *tmpb, *cres;   // [np][n] canonical bit-reversed, [np][n] coset evaluations, [n], [n], [rho*n]
    PlonkCosets<FrP> cosets;
    std::vector<PlonkConsts> hK;                   // [rho]: the proof's constants on every coset, and their place on the device
    PlonkConsts* dK;
    PlonkBatchPtrs B;                              // where the constraint kernel reads each polynomial: work_of(p), no per-proof stride
    uint32_t* canon_of(int p) const { return canon + (size_t)p * n * 8; }
    uint32_t* work_of(int p) const { return work + (size_t)p * n * 8; }

    // cosets.stage and hK die with the run: no copy from them may still be queued when a driver returns early
    ~PlonkRun() {
        if (ctx) hipStreamSynchronize(st);
    }

    int begin(Domain* dom0, Domain* dom1, uint32_t nb_bsb) {
        d0 = dom0, d1 = dom1, ctx = d0->ctx, st = ctx->stream, n = d0->n;
        GA_CHECK(cosets.build(d0, d1, nb_bsb));
        rho = cosets.rho;
        np = PLONK_NB_FIXED + 2 * (int)nb_bsb;
        blocks = (unsigned)((n + 255) / 256);
        GA_CHECK(ctx->scratch_get("plonk_canon", (size_t)np * n * 32, (void**)&canon));
        GA_CHECK(ctx->scratch_get("plonk_work", (size_t)np * n * 32, (void**)&work));
        GA_CHECK(ctx->scratch_get("plonk_inv", n * 32, (void**)&invb));
        GA_CHECK(ctx->scratch_get("plonk_tmp", n * 32, (void**)&tmpb));
        GA_CHECK(ctx->scratch_get("plonk_cres", d1->n * 32, (void**)&cres));
        GA_CHECK(ctx->scratch_get("plonk_qb_consts", rho * sizeof(PlonkConsts), (void**)&dK));
        memset(&B, 0, sizeof(B));
        B.P.nb_bsb = (int)nb_bsb;
        for (int p = 0; p < np; p++) B.P.p[p] = work_of(p);
        return GA_OK;
    }

    // polynomial p of A to canonical coefficients in bit-reversed order (canon_of(p)), once per driver call
    int to_canonical(const PlonkQuotientArgs& A, int p) {
        uint32_t *dst = canon_of(p), *stage = work_of(p);
        const bool lag = (A.lagrange_mask >> p) & 1;
        {
            StageTimer tm(ctx, "plonk_h2d");
            GA_HIP_CHECK(hipMemcpyAsync(lag ? dst : stage, A.polys[p], n * 32, A.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        }
        if (lag)   // Lagrange regular -> canonical bit-reversed: inverse DIF with the 1/n (p.ToCanonical, prove.go:1036)
            return ntt_run<FrP>(d0, dst, /*inverse=*/true, /*dit=*/false, scale_none(), scale_const(d0->ninv));
        StageTimer tm(ctx, "plonk_bitrev");
        hipLaunchKernelGGL((fr_bitrev_copy_kernel<FrP>), dim3(blocks), dim3(256), 0, st, dst, stage, n, d0->logn);
        GA_KERNEL_CHECK();
        return GA_OK;
    }

    // the proof's constants on every coset (the challenges, the blinding coefficients times (coset^n - 1), the images sh[]), uploaded once
    int proof_consts(const PlonkQuotientArgs& A) {
        hK = cosets.K;
        for (uint64_t i = 0; i < rho; i++) plonk_proof_consts<FrP>(hK[i], A, cosets.cexp[i]);
        GA_HIP_CHECK(hipMemcpyAsync(dK, hK.data(), rho * sizeof(PlonkConsts), hipMemcpyHostToDevice, st));
        return GA_OK;
    }

    // dst = evaluations of polynomial p on coset i: one out-of-place forward DIT over the coset's twiddle table
    int eval_on_coset(uint64_t i, int p, uint32_t* dst) {
        return ntt_run<FrP>(d0, dst, /*inverse=*/false, /*dit=*/true, scale_none(), scale_none(), canon_of(p), cosets.tw[i]);
    }

    // out[j] = 1 / (x_j - 1) over coset i
    int inv_x_minus_one(uint64_t i, uint32_t* out) {
        StageTimer tm(ctx, "plonk_batch_inverse");
        hipLaunchKernelGGL((plonk_x_minus_one_kernel<FrP>), dim3(blocks), dim3(256), 0, st, out, cosets.x.lo(i), cosets.x.hi(i), NTT_POW_LO_BITS, n);
        hipLaunchKernelGGL((fr_batch_inverse_kernel<FrP>), dim3((unsigned)((plonk_inverse_threads(n) + 63) / 64)), dim3(64), 0, st, out, tmpb, n);
        GA_KERNEL_CHECK();
        return GA_OK;
    }

    // the constraints of coset i, from the evaluations B.P and 1/(x-1), into their block of cres (one proof: grid y = 1)
    int constraints(uint64_t i, const uint32_t* inv_xm1) {
        StageTimer tm(ctx, "plonk_constraints");
        hipLaunchKernelGGL((plonk_constraints_kernel<FrP, PLONK_LAZY<FrP>>), dim3((unsigned)((n + 127) / 128), 1), dim3(128), 0, st, B,
                           (const PlonkConsts*)(dK + i), cosets.x.lo(i), cosets.x.hi(i), NTT_POW_LO_BITS, inv_xm1,
                           cres + cosets.block(i) * n * 8, (uint64_t)0, n, d0->logn);
        GA_KERNEL_CHECK();
        return GA_OK;
    }

    // a.ToCanonical(bigDomain).ToRegular() from LagrangeCoset/BitReverse (prove.go:1319): inverse DIT on the coset, then h leaves
    int finish(const PlonkQuotientArgs& A, void* h_out) {
        GA_CHECK(ntt_fft<FrP>(d1, cres, GA_FFT_INVERSE, GA_DIT, 1));
        {
            StageTimer tm(ctx, "plonk_d2h");
            GA_HIP_CHECK(hipMemcpyAsync(h_out, cres, d1->n * 32, A.on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
        }
        GA_HIP_CHECK(hipStreamSynchronize(st));
        return GA_OK;
    }
};

// Every polynomial per call.
template <class FrP>
int plonk_quotient(Domain* d0, Domain* d1, const PlonkQuotientArgs& A, void* h_out) {
    PlonkRun<FrP> R;
    GA_CHECK(R.begin(d0, d1, A.nb_bsb));
    for (int p = 0; p < R.np; p++) GA_CHECK(R.to_canonical(A, p));
    GA_CHECK(R.proof_consts(A));
    for (uint64_t i = 0; i < R.rho; i++) {
        for (int p = 0; p < R.np; p++) GA_CHECK(R.eval_on_coset(i, p, R.work_of(p)));
        GA_CHECK(R.inv_x_minus_one(i, R.invb));
        GA_CHECK(R.constraints(i, R.invb));
    }
    return R.finish(A, h_out);
}

// The key: the circuit constants of A on every coset and 1/(x-1) per coset; no quotient.
template <class FrP>
int plonk_fixed_create(Domain* d0, Domain* d1, const PlonkQuotientArgs& A, PlonkFixed** out) {
    PlonkRun<FrP> R;
    GA_CHECK(R.begin(d0, d1, A.nb_bsb));
    const std::vector<int> fixed = plonk_ids(R.np, true);
    std::unique_ptr<PlonkFixed, void (*)(PlonkFixed*)> fx(new PlonkFixed(), plonk_fixed_destroy);
    fx->d0 = d0;
    fx->d1 = d1;
    fx->nb_bsb = A.nb_bsb;
    std::fill(std::begin(fx->slot), std::end(fx->slot), -1);
    for (int p : fixed) fx->slot[p] = fx->nslots++;
    const size_t ev = (size_t)R.rho * fx->nslots * R.n * 32, iv = (size_t)R.rho * R.n * 32;
    if (device_malloc((void**)&fx->evals, ev) != hipSuccess || device_malloc((void**)&fx->inv_xm1, iv) != hipSuccess) {
        set_error("plonk key: hipMalloc of %zu bytes failed", ev + iv);
        return GA_ERR_NOMEM;
    }
    for (int p : fixed) GA_CHECK(R.to_canonical(A, p));
    for (uint64_t i = 0; i < R.rho; i++) {
        for (int p : fixed) GA_CHECK(R.eval_on_coset(i, p, fx->evals_of(i, p)));
        GA_CHECK(R.inv_x_minus_one(i, fx->inv_xm1_of(i)));
    }
    GA_HIP_CHECK(hipStreamSynchronize(R.st));
    *out = fx.release();
    return GA_OK;
}

// out[i] = sum_k s_k * v_k[i]: the folding of kzg.BatchOpenSinglePoint and the linear combinations of the linearised polynomial
// (backend/plonk/bn254/prove.go:1352-1460) as one pass over the vectors
constexpr int LINCOMB_MAX = 16;
struct LinCombArgs {
    const uint32_t* v[LINCOMB_MAX];
    uint32_t s[LINCOMB_MAX][8];
    int k;
};
template <class FrP>
__global__ void fr_lincomb_kernel(LinCombArgs A, uint32_t* __restrict__ out, uint64_t n) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fe<FrP> acc = fe_zero<FrP>();
    for (int k = 0; k < A.k; k++) acc = add(acc, mul_val(load_fe<FrP>(A.v[k] + i * 8), plonk_c<FrP>(A.s[k])));
    store_fe(out + i * 8, acc);
}
template <class FrP>
int fr_lincomb(Ctx* ctx, uint64_t n, int k, const void* const* vecs, const void* scalars, void* out, bool on_device) {
    if (k < 1 || k > LINCOMB_MAX) {
        set_error("linear combination of %d vectors: 1..%d supported per call", k, LINCOMB_MAX);
        return GA_ERR_INVALID;
    }
    if (n == 0) return GA_OK;
    hipStream_t st = ctx->stream;
    LinCombArgs A;
    memset(&A, 0, sizeof(A));
    A.k = k;
    uint32_t *stage = nullptr, *dout = (uint32_t*)out;
    if (!on_device) {
        GA_CHECK(ctx->scratch_get("lincomb_in", (size_t)(k + 1) * n * 32, (void**)&stage));
        dout = stage + (size_t)k * n * 8;
    }
    for (int j = 0; j < k; j++) {
        memcpy(A.s[j], (const char*)scalars + 32 * j, 32);
        if (on_device) {
            A.v[j] = (const uint32_t*)vecs[j];
        } else {
            GA_HIP_CHECK(hipMemcpyAsync(stage + (size_t)j * n * 8, vecs[j], n * 32, hipMemcpyHostToDevice, st));
            A.v[j] = stage + (size_t)j * n * 8;
        }
    }
    {
        StageTimer tm(ctx, "fr_lincomb");
        hipLaunchKernelGGL((fr_lincomb_kernel<FrP>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A, dout, n);
        GA_KERNEL_CHECK();
    }
    if (!on_device) GA_HIP_CHECK(hipMemcpyAsync(out, dout, n * 32, hipMemcpyDeviceToHost, st));
    GA_HIP_CHECK(hipStreamSynchronize(st));
    return GA_OK;
}

// fr.BatchInvert on a vector (host or device memory), in place
template <class FrP>
int fr_batch_inverse(Ctx* ctx, void* v, uint64_t n, bool on_device) {
    if (n == 0) return GA_OK;
    uint32_t *buf, *tmp;
    GA_CHECK(ctx->scratch_get("plonk_inv", n * 32, (void**)&buf));
    GA_CHECK(ctx->scratch_get("plonk_tmp", n * 32, (void**)&tmp));
    hipStream_t st = ctx->stream;
    uint32_t* d = on_device ? (uint32_t*)v : buf;
    if (!on_device) GA_HIP_CHECK(hipMemcpyAsync(buf, v, n * 32, hipMemcpyHostToDevice, st));
    {
        StageTimer tm(ctx, "plonk_batch_inverse");
        hipLaunchKernelGGL((fr_batch_inverse_kernel<FrP>), dim3((unsigned)((plonk_inverse_threads(n) + 63) / 64)), dim3(64), 0, st, d, tmp, n);
        GA_KERNEL_CHECK();
    }
    if (!on_device) GA_HIP_CHECK(hipMemcpyAsync(v, buf, n * 32, hipMemcpyDeviceToHost, st));
    GA_HIP_CHECK(hipStreamSynchronize(st));
    return GA_OK;
}

// entries of a device-resident permutation outside [0, 3n) would index the identity tables out of bounds
static __global__ void plonk_perm_check_kernel(const int64_t* __restrict__ perm, uint64_t n3, uint32_t* __restrict__ bad) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n3 && (perm[i] < 0 || (uint64_t)perm[i] >= n3)) atomicAdd(bad, 1u);
}

// ---- the per-curve calls declared in common.hip.h: C::FrP for the drivers above (instantiated with those of plonk_batch.hip.h) ----
template <class C>
int plonk_domain_quotient(Domain* d0, Domain* d1, const PlonkQuotientArgs& args, void* h_out) {
    return plonk_quotient<typename C::FrP>(d0, d1, args, h_out);
}
template <class C>
int plonk_domain_fixed_create(Domain* d0, Domain* d1, const PlonkQuotientArgs& args, PlonkFixed** out) {
    return plonk_fixed_create<typename C::FrP>(d0, d1, args, out);
}
template <class C>
int fr_vec_batch_inverse(Ctx* ctx, void* v, uint64_t n, bool on_device) {
    return fr_batch_inverse<typename C::FrP>(ctx, v, n, on_device);
}
template <class C>
int fr_vec_lincomb(Ctx* ctx, uint64_t n, int k, const void* const* vecs, const void* scalars, void* out, bool on_device) {
    return fr_lincomb<typename C::FrP>(ctx, n, k, vecs, scalars, out, on_device);
}

}  // namespace ga

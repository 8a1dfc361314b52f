// Pairing products: ok[g] = ( prod_{i in group g} e(P_i, Q_i) == 1 ) for n (G1Affine, G2Affine) pairs cut into groups -- what
// gnark-crypto's curve.PairingCheck decides for the Groth16 verifier (backend/groth16/<curve>/verify.go:128-139), for
// pedersen.BatchVerifyMultiVk (verify.go:104-112), for kzg.Verify / BatchVerifyMultiPoints, for the SameRatio pairings of mpcsetup's
// Verify, and -- with the group's value written out -- vk.Precompute's e(alpha, beta) (verify.go:70-73 reads vk.e).
//
// Arithmetic, all on the exact layer (field.hip.h, the Fe2 of ec.hip.h):
//   tower     gnark's: Fp6 = Fp2[v]/(v^3 - xi), Fp12 = Fp6[w]/(w^2 - v), xi = 9 + u (BN254), 1 + u (BLS12-381); memory image = E12
//             {C0{B0,B1,B2}, C1{B0,B1,B2}}.  In powers of w (w^6 = xi) the Fp2 at C_i.B_j is the coefficient of w^(2j + i).
//   lines     the running point R = (X, Y, Z) stays on the twist in homogeneous projective coordinates: no inversion in the loop.
//             Every line is three Fp2 values (cy yP, cx xP, c0), known up to a factor in Fp2, which the final exponentiation kills:
//               doubling   cy = -2YZ, cx = 3X^2, c0 = 3b'Z^2 - Y^2;  X3 = 2XY(B - F), Y3 = (B + F)^2 - 12E^2, Z3 = 8BYZ
//                          with B = Y^2, E = 3b'Z^2, F = 3E (Costello-Lange-Naehrig, scaled by 4: no halving)
//               addition   of the affine (x2, y2): theta = Y - y2 Z, lambda = X - x2 Z; cy = -lambda, cx = theta, c0 = y2 lambda - theta x2
//             D-type twist (BN254):     cy yP + cx xP w + c0 w^3   -> C0.B0, C1.B0, C1.B1
//             M-type twist (BLS12-381): c0 + cx xP w^2 + cy yP w^3 -> C0.B0, C0.B1, C1.B1
//             and f * line is 13 Fp2 products (pairing_mul_line) instead of 18.
//   loop      BLS12-381: over |x0| = 0xd201000000010000, then a conjugation (x0 < 0).  BN254: the optimal-ate loop over 6 x0 + 2
//             (65 bits) and the two lines through pi(Q), -pi^2(Q) (the psi constants of check_points.hip.h): half the length of the
//             plain ate loop over 6 x0^2.  The loop count is a compile-time constant: every lane of every wave takes the same
//             sequence, and nothing inside it is branched on.  A pair with (0,0) on either side contributes 1.
//   exponent  e = (p^6 - 1)(p^2 + 1) h with the hard part
//               BLS12-381  h = 3 (p^4 - p^2 + 1)/r = (x0 - 1)^2 (x0 + p)(x0^2 + p^2 - 1) + 3
//               BN254      h = l0 + l1 p + l2 p^2 + p^3,  l2 = 6x0^2 + 1, l1 = -36x0^3 - 18x0^2 - 12x0 + 1, l0 = -36x0^3 - 30x0^2 - 18x0 - 2
//                          (a multiple of (p^4 - p^2 + 1)/r by a cofactor prime to r)
//             by the seed chains with cyclotomic squarings (Granger-Scott).  gt[g] is prod f_i to that power: the library's own
//             normalisation of e, consistent with itself and not promised to equal gnark-crypto's Pair.
//   invalid   inv(0) = 0 (Fermat).  A Q of small order sends R to Z = 0, the lines and f to 0, and the lane ends with gt = 0: "not 1".
//
// On the context's work stream, one host synchronisation, per chunk of pairs (GA_PAIRING_CHUNK):
//   1. pairing_miller_kernel    one lane per pair, one-wave workgroups; f lives in the lane's LDS column between the steps (12 N words
//                               per lane), the running point and the line in registers.
//   2. pairing_product_kernel   one lane per segment of at most PAIRING_SEGMENT factors (rows of csr_plan.hip.h: the groups cut to
//                               the chunk); a longer group is multiplied as partial products, level by level.  The product of a group's
//                               part of the chunk is multiplied into the group's accumulator (1 at the start: an empty group is 1).
// then 3. pairing_final_kernel  one lane per group: the final exponentiation, ok[g], gt[g], and the call's two counters.
#pragma once
#include <vector>

#include "csr_plan.hip.h"   // CsrLevels, csr_cut_levels; SPARSE_FINAL
#include "ec.hip.h"         // Fe2, Affine
#include "keyio.hip.h"      // CurveB
#include "vec_call.hip.h"

namespace ga {

constexpr uint64_t PAIRING_DEFAULT_CHUNK = 1ull << 18;   // pairs per pass: one Fp12 each (96 or 144 MiB)
constexpr uint32_t PAIRING_SEGMENT = 16;                 // factors, or partial products, per lane of the group products
constexpr unsigned PAIRING_THREADS = 64;
constexpr unsigned PAIRING_MAX_BLOCKS = 1024;            // workgroups of a launch (grid-stride beyond)

// per base field: xi = XI_A + u, the twist type, the loop count (bit 64 implied when LOOP_TOP64) and |x0|
template <class P> struct PairingCurve;
template <> struct PairingCurve<BN254_Fp> {
    static constexpr int XI_A = 9;
    static constexpr bool MTWIST = false, OPTIMAL_ATE = true, LOOP_TOP64 = true, NEG_SEED = false;
    static constexpr uint64_t LOOP = 11347224129447541672ull;   // 6 x0 + 2 - 2^64
    static constexpr uint64_t SEED = 4965661367192848881ull;
};
template <> struct PairingCurve<BLS12_381_Fp> {
    static constexpr int XI_A = 1;
    static constexpr bool MTWIST = true, OPTIMAL_ATE = false, LOOP_TOP64 = false, NEG_SEED = true;
    static constexpr uint64_t LOOP = 0xd201000000010000ull;
    static constexpr uint64_t SEED = 0xd201000000010000ull;
};

template <class P> struct Fe6 { Fe2<P> b0, b1, b2; };    // b0 + b1 v + b2 v^2  (gnark E6{B0, B1, B2})
template <class P> struct Fe12 { Fe6<P> c0, c1; };       // c0 + c1 w          (gnark E12{C0, C1})

// ---- Fp2 helpers ------------------------------------------------------------------------------------------------------------------
template <class P> GA_HD Fe2<P> pr_conj(const Fe2<P>& a) { return {a.c0, neg(a.c1)}; }
template <class P> GA_HD Fe2<P> pr_mul_fp(const Fe2<P>& a, const Fe<P>& k) { return {mul(a.c0, k), mul(a.c1, k)}; }
template <class P> GA_HD Fe2<P> pr_triple(const Fe2<P>& a) { return add(dbl(a), a); }
// a xi = (A a0 - a1) + (A a1 + a0) u
template <class P>
GA_HD Fe2<P> mul_xi(const Fe2<P>& a) {
    if constexpr (PairingCurve<P>::XI_A == 1) return {sub(a.c0, a.c1), add(a.c0, a.c1)};
    else {
        const Fe<P> n0 = add(dbl(dbl(dbl(a.c0))), a.c0), n1 = add(dbl(dbl(dbl(a.c1))), a.c1);   // 9 a
        return {sub(n0, a.c1), add(n1, a.c0)};
    }
}

// ---- Fp6 ----------------------------------------------------------------------------------------------------------------------------
template <class P> GA_HD Fe6<P> add(const Fe6<P>& a, const Fe6<P>& b) { return {add(a.b0, b.b0), add(a.b1, b.b1), add(a.b2, b.b2)}; }
template <class P> GA_HD Fe6<P> sub(const Fe6<P>& a, const Fe6<P>& b) { return {sub(a.b0, b.b0), sub(a.b1, b.b1), sub(a.b2, b.b2)}; }
template <class P> GA_HD Fe6<P> neg(const Fe6<P>& a) { return {neg(a.b0), neg(a.b1), neg(a.b2)}; }
template <class P> GA_HD Fe6<P> dbl(const Fe6<P>& a) { return {dbl(a.b0), dbl(a.b1), dbl(a.b2)}; }
template <class P> GA_HD bool eq(const Fe6<P>& a, const Fe6<P>& b) { return eq(a.b0, b.b0) & eq(a.b1, b.b1) & eq(a.b2, b.b2); }
template <class P> GA_HD Fe6<P> mul_v(const Fe6<P>& a) { return {mul_xi(a.b2), a.b0, a.b1}; }

// Karatsuba: 6 Fp2 products
template <class P>
GA_HD_CALL Fe6<P> mul(const Fe6<P>& a, const Fe6<P>& b) {
    const Fe2<P> t0 = mul(a.b0, b.b0), t1 = mul(a.b1, b.b1), t2 = mul(a.b2, b.b2);
    const Fe2<P> m12 = mul(add(a.b1, a.b2), add(b.b1, b.b2)), m01 = mul(add(a.b0, a.b1), add(b.b0, b.b1)), m02 = mul(add(a.b0, a.b2), add(b.b0, b.b2));
    return {add(mul_xi(sub(sub(m12, t1), t2)), t0), add(sub(sub(m01, t0), t1), mul_xi(t2)), add(sub(sub(m02, t0), t2), t1)};
}
// a (c0 + c1 v): 5 products;  a (c1 v): 3;  a c0: 3
template <class P>
GA_HD_CALL Fe6<P> mul_by_01(const Fe6<P>& a, const Fe2<P>& c0, const Fe2<P>& c1) {
    const Fe2<P> t0 = mul(a.b0, c0), t1 = mul(a.b1, c1);
    const Fe2<P> r0 = add(mul_xi(sub(mul(add(a.b1, a.b2), c1), t1)), t0);
    const Fe2<P> r1 = sub(sub(mul(add(a.b0, a.b1), add(c0, c1)), t0), t1);
    const Fe2<P> r2 = add(sub(mul(add(a.b0, a.b2), c0), t0), t1);
    return {r0, r1, r2};
}
template <class P>
GA_HD Fe6<P> mul_by_1(const Fe6<P>& a, const Fe2<P>& c1) { return {mul_xi(mul(a.b2, c1)), mul(a.b0, c1), mul(a.b1, c1)}; }
template <class P>
GA_HD Fe6<P> mul_by_0(const Fe6<P>& a, const Fe2<P>& c0) { return {mul(a.b0, c0), mul(a.b1, c0), mul(a.b2, c0)}; }

// (0 -> 0: the Fp2 inverse of 0 is 0)
template <class P>
GA_HD_CALL Fe6<P> inv(const Fe6<P>& a) {
    const Fe2<P> A = sub(sqr(a.b0), mul_xi(mul(a.b1, a.b2)));
    const Fe2<P> B = sub(mul_xi(sqr(a.b2)), mul(a.b0, a.b1));
    const Fe2<P> C = sub(sqr(a.b1), mul(a.b0, a.b2));
    const Fe2<P> t = inv(add(mul(a.b0, A), mul_xi(add(mul(a.b2, B), mul(a.b1, C)))));
    return {mul(A, t), mul(B, t), mul(C, t)};
}

// ---- Fp12 ---------------------------------------------------------------------------------------------------------------------------
template <class P>
GA_HD Fe12<P> fe12_one() {
    const Fe2<P> z = FieldTraits<Fe2<P>>::zero();
    return {{FieldTraits<Fe2<P>>::one(), z, z}, {z, z, z}};
}
template <class P> GA_HD bool eq(const Fe12<P>& a, const Fe12<P>& b) { return eq(a.c0, b.c0) & eq(a.c1, b.c1); }
template <class P> GA_HD Fe12<P> conj(const Fe12<P>& a) { return {a.c0, neg(a.c1)}; }

// Karatsuba over Fp6: 18 Fp2 products
template <class P>
GA_HD_CALL Fe12<P> mul(const Fe12<P>& a, const Fe12<P>& b) {
    const Fe6<P> t0 = mul(a.c0, b.c0), t1 = mul(a.c1, b.c1);
    const Fe6<P> m = mul(add(a.c0, a.c1), add(b.c0, b.c1));
    return {add(t0, mul_v(t1)), sub(sub(m, t0), t1)};
}
// complex squaring: 12 Fp2 products
template <class P>
GA_HD_CALL Fe12<P> sqr(const Fe12<P>& a) {
    const Fe6<P> t = mul(a.c0, a.c1);
    const Fe6<P> m = mul(add(a.c0, a.c1), add(a.c0, mul_v(a.c1)));
    return {sub(sub(m, t), mul_v(t)), dbl(t)};
}
// 1 / (c0 + c1 w) = (c0 - c1 w) / (c0^2 - v c1^2); 0 -> 0
template <class P>
GA_HD_CALL Fe12<P> inv(const Fe12<P>& a) {
    const Fe6<P> t = inv(sub(mul(a.c0, a.c0), mul_v(mul(a.c1, a.c1))));
    return {mul(a.c0, t), neg(mul(a.c1, t))};
}

// the squaring of an element of the cyclotomic subgroup (Granger-Scott), 9 Fp2 squarings; x0..x5 = C0.B0, C0.B1, C0.B2, C1.B0, C1.B1, C1.B2:
//   (3 x4^2 xi + 3 x0^2 - 2 x0, 3 x2^2 xi + 3 x3^2 - 2 x1, 3 x5^2 xi + 3 x1^2 - 2 x2, 6 x1 x5 xi + 2 x3, 6 x0 x4 + 2 x4, 6 x2 x3 + 2 x5)
template <class P>
GA_HD_CALL Fe12<P> cyclotomic_sqr(const Fe12<P>& x) {
    Fe2<P> t0 = sqr(x.c1.b1), t1 = sqr(x.c0.b0), t2 = sqr(x.c0.b2), t3 = sqr(x.c1.b0), t4 = sqr(x.c1.b2), t5 = sqr(x.c0.b1);
    const Fe2<P> t6 = sub(sub(sqr(add(x.c1.b1, x.c0.b0)), t0), t1);            // 2 x4 x0
    const Fe2<P> t7 = sub(sub(sqr(add(x.c0.b2, x.c1.b0)), t2), t3);            // 2 x2 x3
    const Fe2<P> t8 = mul_xi(sub(sub(sqr(add(x.c1.b2, x.c0.b1)), t4), t5));    // 2 x5 x1 xi
    t0 = add(mul_xi(t0), t1);
    t2 = add(mul_xi(t2), t3);
    t4 = add(mul_xi(t4), t5);
    Fe12<P> z;
    z.c0.b0 = add(dbl(sub(t0, x.c0.b0)), t0);
    z.c0.b1 = add(dbl(sub(t2, x.c0.b1)), t2);
    z.c0.b2 = add(dbl(sub(t4, x.c0.b2)), t4);
    z.c1.b0 = add(dbl(add(t8, x.c1.b0)), t8);
    z.c1.b1 = add(dbl(add(t6, x.c1.b1)), t6);
    z.c1.b2 = add(dbl(add(t7, x.c1.b2)), t7);
    return z;
}

// a^(p^K), K = 1, 2, 3: the coefficient of w^i goes to its own p^K-th power (a conjugation for odd K) times xi^(i (p^K - 1)/6)
// (constants.h FROB1 / FROB2 / FROB3, tools/gen_constants.py pairing_constants)
template <int K, int I, class P>
GA_HD Fe2<P> frobenius_coeff(const Fe2<P>& a) {
    const Fe2<P> c = (K & 1) ? pr_conj(a) : a;
    if constexpr (I == 0) return c;
    else if constexpr (K == 2) return pr_mul_fp(c, fe_const<P>(P::FROB2[I - 1]));
    else if constexpr (K == 1) return mul(c, Fe2<P>{fe_const<P>(P::FROB1[2 * (I - 1)]), fe_const<P>(P::FROB1[2 * (I - 1) + 1])});
    else return mul(c, Fe2<P>{fe_const<P>(P::FROB3[2 * (I - 1)]), fe_const<P>(P::FROB3[2 * (I - 1) + 1])});
}
template <int K, class P>
GA_HD_CALL Fe12<P> frobenius(const Fe12<P>& a) {
    return {{frobenius_coeff<K, 0>(a.c0.b0), frobenius_coeff<K, 2>(a.c0.b1), frobenius_coeff<K, 4>(a.c0.b2)},
            {frobenius_coeff<K, 1>(a.c1.b0), frobenius_coeff<K, 3>(a.c1.b1), frobenius_coeff<K, 5>(a.c1.b2)}};
}

// f times the line (ly = cy yP, lx = cx xP, l0 = c0) at the positions of the twist type: 13 Fp2 products
template <class P>
GA_HD_CALL Fe12<P> pairing_mul_line(const Fe12<P>& f, const Fe2<P>& ly, const Fe2<P>& lx, const Fe2<P>& l0) {
    Fe6<P> t0, t1, m;
    if constexpr (PairingCurve<P>::MTWIST) {   // (l0, lx, 0) + (0, ly, 0) w
        t0 = mul_by_01(f.c0, l0, lx);
        t1 = mul_by_1(f.c1, ly);
        m = mul_by_01(add(f.c0, f.c1), l0, add(lx, ly));
    } else {                                   // (ly, 0, 0) + (lx, l0, 0) w
        t0 = mul_by_0(f.c0, ly);
        t1 = mul_by_01(f.c1, lx, l0);
        m = mul_by_01(add(f.c0, f.c1), add(ly, lx), l0);
    }
    return {add(t0, mul_v(t1)), sub(sub(m, t0), t1)};
}

// ---- the Miller loop --------------------------------------------------------------------------------------------------------------
template <class P> struct PairingPoint { Fe2<P> x, y, z; };
template <class P> struct PairingLine { Fe2<P> cy, cx, c0; };

// R <- 2R and the tangent at R: 4 products, 6 squarings
template <class P>
GA_HD_CALL PairingLine<P> pairing_double_step(PairingPoint<P>& r) {
    const Fe2<P> B = sqr(r.y), C = sqr(r.z);
    const Fe2<P> E = mul(pr_triple(C), CurveB<Fe2<P>>::get()), F = pr_triple(E);
    const Fe2<P> H = sub(sub(sqr(add(r.y, r.z)), B), C);   // 2YZ
    const PairingLine<P> l{neg(H), pr_triple(sqr(r.x)), sub(E, B)};
    const Fe2<P> BF = add(B, F), E2 = dbl(E);
    r.x = mul(dbl(mul(r.x, r.y)), sub(B, F));
    r.y = sub(sqr(BF), pr_triple(sqr(E2)));
    r.z = dbl(dbl(mul(B, H)));
    return l;
}
// R <- R + Q for the affine Q and the chord through them: 11 products, 2 squarings
template <class P>
GA_HD_CALL PairingLine<P> pairing_add_step(PairingPoint<P>& r, const Affine<Fe2<P>>& q) {
    const Fe2<P> theta = sub(r.y, mul(q.y, r.z)), lambda = sub(r.x, mul(q.x, r.z));
    const PairingLine<P> l{neg(lambda), theta, sub(mul(q.y, lambda), mul(theta, q.x))};
    const Fe2<P> C = sqr(theta), D = sqr(lambda), E = mul(lambda, D), G = mul(r.x, D);
    const Fe2<P> H = sub(add(E, mul(r.z, C)), dbl(G));
    r.x = mul(lambda, H);
    r.y = sub(mul(theta, sub(G, H)), mul(E, r.y));
    r.z = mul(r.z, E);
    return l;
}

// the lane's Fp12 in LDS: word k of lane t at lds[k * PAIRING_THREADS + t] (no bank conflicts)
template <class P>
struct LdsFe12 {
    static constexpr int NW = 12 * P::N;
    uint32_t* col;
    __device__ __forceinline__ Fe12<P> get() const {
        Fe12<P> f;
        uint32_t* w = reinterpret_cast<uint32_t*>(&f);
#pragma unroll
        for (int k = 0; k < NW; k++) w[k] = col[k * PAIRING_THREADS];
        return f;
    }
    __device__ __forceinline__ void put(const Fe12<P>& f) const {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(&f);
#pragma unroll
        for (int k = 0; k < NW; k++) col[k * PAIRING_THREADS] = w[k];
    }
};

template <class P>
__device__ __forceinline__ void pairing_apply_line(const LdsFe12<P>& F, const PairingLine<P>& l, const Affine<Fe<P>>& p) {
    F.put(pairing_mul_line(F.get(), pr_mul_fp(l.cy, p.y), pr_mul_fp(l.cx, p.x), l.c0));
}

// f_{loop, Q}(P) (and the two closing lines of the optimal-ate pairing); neither point is (0,0)
template <class P>
__device__ __forceinline__ Fe12<P> pairing_miller_loop(const Affine<Fe<P>>& p, const Affine<Fe2<P>>& q, const LdsFe12<P>& F) {
    typedef PairingCurve<P> PC;
    PairingPoint<P> r{q.x, q.y, FieldTraits<Fe2<P>>::one()};
    F.put(fe12_one<P>());
    constexpr int TOP = PC::LOOP_TOP64 ? 64 : 63 - __builtin_clzll(PC::LOOP);
#pragma unroll 1
    for (int b = TOP - 1; b >= 0; b--) {
        F.put(sqr(F.get()));
        pairing_apply_line(F, pairing_double_step(r), p);
        if ((PC::LOOP >> b) & 1) pairing_apply_line(F, pairing_add_step(r, q), p);
    }
    if constexpr (PC::OPTIMAL_ATE) {
        const Fe2<P> cx{fe_const<P>(P::PSI_X0), fe_const<P>(P::PSI_X1)}, cy{fe_const<P>(P::PSI_Y0), fe_const<P>(P::PSI_Y1)};
        const Affine<Fe2<P>> q1{mul(pr_conj(q.x), cx), mul(pr_conj(q.y), cy)};                                              // pi(Q)
        const Affine<Fe2<P>> q2{pr_mul_fp(q.x, fe_const<P>(P::PSI2_X)), neg(pr_mul_fp(q.y, fe_const<P>(P::PSI2_Y)))};       // -pi^2(Q)
        pairing_apply_line(F, pairing_add_step(r, q1), p);
        pairing_apply_line(F, pairing_add_step(r, q2), p);
    }
    const Fe12<P> f = F.get();
    return PC::NEG_SEED ? conj(f) : f;
}

template <class P>
__global__ void __launch_bounds__(PAIRING_THREADS)
pairing_miller_kernel(const Affine<Fe<P>>* __restrict__ ps, const Affine<Fe2<P>>* __restrict__ qs, uint32_t n, Fe12<P>* __restrict__ out) {
    __shared__ uint32_t lds[LdsFe12<P>::NW * PAIRING_THREADS];
    const LdsFe12<P> F{lds + threadIdx.x};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const Affine<Fe<P>> p = load_pod<Affine<Fe<P>>>(&ps[i]);
        const Affine<Fe2<P>> q = load_pod<Affine<Fe2<P>>>(&qs[i]);
        if (is_inf(p) | is_inf(q)) {
            store_pod(&out[i], fe12_one<P>());
            continue;
        }
        store_pod(&out[i], pairing_miller_loop<P>(p, q, F));
    }
}

// ---- group products ----------------------------------------------------------------------------------------------------------------
// segs: {first factor, factors, destination} per segment; a final segment multiplies its product into acc[row_base + row]
template <class P>
__global__ void __launch_bounds__(PAIRING_THREADS)
pairing_product_kernel(const uint32_t* __restrict__ segs, uint32_t nseg, const Fe12<P>* __restrict__ in, Fe12<P>* __restrict__ part, Fe12<P>* __restrict__ acc,
                       uint32_t row_base) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nseg; i += gridDim.x * blockDim.x) {
        const uint64_t first = segs[3 * (uint64_t)i];
        const uint32_t count = segs[3 * (uint64_t)i + 1], dst = segs[3 * (uint64_t)i + 2];
        Fe12<P>* out = (dst & SPARSE_FINAL) ? &acc[(uint64_t)row_base + (dst & ~SPARSE_FINAL)] : &part[dst];
        Fe12<P> f = (dst & SPARSE_FINAL) ? load_pod<Fe12<P>>(out) : fe12_one<P>();
#pragma unroll 1
        for (uint32_t k = 0; k < count; k++) f = mul(f, load_pod<Fe12<P>>(&in[first + k]));
        store_pod(out, f);
    }
}

template <class P>
__global__ void __launch_bounds__(256)
pairing_fill_one_kernel(Fe12<P>* __restrict__ acc, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) store_pod(&acc[i], fe12_one<P>());
}

// ---- the final exponentiation --------------------------------------------------------------------------------------------------------
// a^|x0| for a in the cyclotomic subgroup
template <class P>
GA_HD_CALL Fe12<P> pairing_exp_seed(const Fe12<P>& a) {
    constexpr uint64_t S = PairingCurve<P>::SEED;
    constexpr int TOP = 63 - __builtin_clzll(S);
    Fe12<P> r = a;
    for (int b = TOP - 1; b >= 0; b--) {
        r = cyclotomic_sqr(r);
        if ((S >> b) & 1) r = mul(r, a);
    }
    return r;
}

template <class P>
GA_HD_CALL Fe12<P> pairing_final_exp(const Fe12<P>& f0) {
    // easy part: (p^6 - 1)(p^2 + 1); from here on the inverse is the conjugate
    Fe12<P> f = mul(conj(f0), inv(f0));
    f = mul(frobenius<2>(f), f);
    if constexpr (PairingCurve<P>::NEG_SEED) {
        // BLS12-381, x0 = -|x0|: f^((x0 - 1)^2 (x0 + p)(x0^2 + p^2 - 1) + 3)
        Fe12<P> y = conj(mul(pairing_exp_seed(f), f));                        // f^(x0 - 1)
        y = conj(mul(pairing_exp_seed(y), y));                                // ^(x0 - 1)
        const Fe12<P> u = mul(conj(pairing_exp_seed(y)), frobenius<1>(y));    // y^(x0 + p)
        const Fe12<P> v = mul(mul(pairing_exp_seed(pairing_exp_seed(u)), frobenius<2>(u)), conj(u));   // u^(x0^2 + p^2 - 1)
        return mul(v, mul(cyclotomic_sqr(f), f));
    } else {
        // BN254, x0 > 0: y0 y1^2 y2^6 y3^12 y4^18 y5^30 y6^36 (Scott et al.) = f^(l0 + l1 p + l2 p^2 + p^3)
        const Fe12<P> a = pairing_exp_seed(f), b = pairing_exp_seed(a), c = pairing_exp_seed(b);
        const Fe12<P> y0 = mul(mul(frobenius<1>(f), frobenius<2>(f)), frobenius<3>(f));
        const Fe12<P> y1 = conj(f), y2 = frobenius<2>(b), y3 = conj(frobenius<1>(a));
        const Fe12<P> y4 = conj(mul(a, frobenius<1>(b))), y5 = conj(b), y6 = conj(mul(c, frobenius<1>(c)));
        Fe12<P> t0 = mul(mul(cyclotomic_sqr(y6), y4), y5);
        Fe12<P> t1 = mul(mul(y3, y5), t0);
        t0 = mul(t0, y2);
        t1 = cyclotomic_sqr(mul(cyclotomic_sqr(t1), t0));
        t0 = cyclotomic_sqr(mul(t1, y1));
        return mul(t0, mul(t1, y0));
    }
}

// the call's counters: groups whose product is not 1, and the complement of the lowest such index (0 = none yet)
struct PairingCounters {
    unsigned long long bad;
    uint32_t first_inv, pad;
};

template <class P>
__global__ void __launch_bounds__(PAIRING_THREADS)
pairing_final_kernel(const Fe12<P>* acc, uint32_t n_groups, uint8_t* __restrict__ ok, Fe12<P>* gt, PairingCounters* __restrict__ cnt) {   // (gt may be acc)
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n_groups; g += gridDim.x * blockDim.x) {
        const Fe12<P> e = pairing_final_exp(load_pod<Fe12<P>>(&acc[g]));
        const bool one = eq(e, fe12_one<P>());
        if (ok) ok[g] = one ? 1 : 0;
        if (gt) store_pod(&gt[g], e);
        if (!one) {
            atomicAdd(&cnt->bad, 1ull);
            atomicMax(&cnt->first_inv, ~g);
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// the groups cut to one chunk of pairs: rows row_base .. row_base + rows - 1 (the empty groups between them included)
struct PairingPass {
    uint64_t first, pairs;
    uint32_t row_base;
    CsrLevels rows;
};

// group_start is valid (abi.hip); forced_chunk: GA_PAIRING_CHUNK (0 = default)
template <class C>
int pairing_run(Ctx* ctx, const void* p_affine, const void* q_affine, size_t n, const uint64_t* group_start, size_t n_groups, unsigned flags, uint8_t* ok,
                void* gt, uint64_t* out2, uint64_t forced_chunk) {
    typedef typename C::FpP P;
    typedef Affine<Fe<P>> A1;
    typedef Affine<Fe2<P>> A2;
    const bool i_dev = (flags & GA_BASES_ON_DEVICE) != 0, o_dev = (flags & GA_RESULT_ON_DEVICE) != 0;
    const uint64_t whole[2] = {0, n};
    if (!group_start) group_start = whole;
    uint64_t chunk = clamp_chunk(forced_chunk, PAIRING_DEFAULT_CHUNK, n);
    if (chunk == 0) chunk = 1;   // (n = 0: the scratch still exists)
    hipStream_t st = ctx->work_stream();

    // the plan of every pass, before anything is launched
    std::vector<PairingPass> passes;
    uint64_t parts[2] = {0, 0}, nsegs = 1;
    {
        size_t g = 0;
        for (uint64_t done = 0; done < n; done += chunk) {
            PairingPass ps;
            ps.first = done;
            ps.pairs = n - done < chunk ? n - done : chunk;
            const uint64_t end = done + ps.pairs;
            while (g < n_groups && group_start[g + 1] <= done) g++;   // groups that ended before this pass
            ps.row_base = (uint32_t)g;
            std::vector<uint64_t> local{0};
            for (size_t h = g; h < n_groups && group_start[h] < end; h++) local.push_back((group_start[h + 1] < end ? group_start[h + 1] : end) - done);
            csr_cut_levels(local.data(), local.size() - 1, PAIRING_SEGMENT, ps.rows);
            uint64_t pp[2];
            ps.rows.part_sizes(pp);
            for (int b = 0; b < 2; b++)
                if (pp[b] > parts[b]) parts[b] = pp[b];
            if (ps.rows.segs.size() / 3 > nsegs) nsegs = ps.rows.segs.size() / 3;
            passes.push_back(std::move(ps));
        }
    }

    // the scratch of the whole call first: an allocation failure leaves nothing in flight
    Fe12<P>*pair_f = nullptr, *acc = nullptr, *part[2] = {nullptr, nullptr};
    uint32_t* segs = nullptr;
    uint8_t* d_ok = nullptr;
    PairingCounters* cnt = nullptr;
    A1* io_p = nullptr;
    A2* io_q = nullptr;
    GA_CHECK(ctx->scratch_get("pairing_values", chunk * sizeof(Fe12<P>), (void**)&pair_f));
    GA_CHECK(ctx->scratch_get("pairing_groups", n_groups * sizeof(Fe12<P>), (void**)&acc));
    GA_CHECK(ctx->scratch_get("pairing_segments", nsegs * 12, (void**)&segs));
    GA_CHECK(ctx->scratch_get("pairing_counters", sizeof(PairingCounters), (void**)&cnt));
    for (int b = 0; b < 2; b++)
        if (parts[b]) GA_CHECK(ctx->scratch_get(b ? "pairing_partial_b" : "pairing_partial_a", parts[b] * sizeof(Fe12<P>), (void**)&part[b]));
    if (ok && !o_dev) GA_CHECK(ctx->scratch_get("pairing_ok", (n_groups + 15) & ~15ull, (void**)&d_ok));
    if (!i_dev) {
        GA_CHECK(ctx->scratch_get("pairing_p", chunk * sizeof(A1), (void**)&io_p));
        GA_CHECK(ctx->scratch_get("pairing_q", chunk * sizeof(A2), (void**)&io_q));
    }
    StreamDrain drain{st};

    GA_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(PairingCounters), st));
    hipLaunchKernelGGL((pairing_fill_one_kernel<P>), dim3((unsigned)((n_groups + 255) / 256)), dim3(256), 0, st, acc, (uint32_t)n_groups);
    GA_KERNEL_CHECK();
    for (const PairingPass& ps : passes) {
        const uint32_t cn = (uint32_t)ps.pairs;
        const A1* sp;
        const A2* sq;
        GA_CHECK(chunk_in(st, i_dev, (const A1*)p_affine, ps.first, cn, io_p, &sp));
        GA_CHECK(chunk_in(st, i_dev, (const A2*)q_affine, ps.first, cn, io_q, &sq));
        GA_HIP_CHECK(hipMemcpyAsync(segs, ps.rows.segs.data(), ps.rows.segs.size() * 4, hipMemcpyHostToDevice, st));
        {
            StageTimer tm(ctx, "pairing_miller");
            hipLaunchKernelGGL((pairing_miller_kernel<P>), dim3(capped_grid(cn, PAIRING_THREADS, PAIRING_MAX_BLOCKS)), dim3(PAIRING_THREADS), 0, st, sp, sq, cn, pair_f);
            GA_KERNEL_CHECK();
        }
        StageTimer tm(ctx, "pairing_product");
        for (size_t l = 0; l < ps.rows.levels.size(); l++) {
            const CsrLevels::Level& lv = ps.rows.levels[l];
            if (lv.nseg == 0) continue;
            const Fe12<P>* from = l == 0 ? pair_f : part[(l - 1) & 1];
            hipLaunchKernelGGL((pairing_product_kernel<P>), dim3(capped_grid(lv.nseg, PAIRING_THREADS, PAIRING_MAX_BLOCKS)), dim3(PAIRING_THREADS), 0, st,
                               (const uint32_t*)(segs + 3 * lv.first), lv.nseg, from, part[l & 1], acc, ps.row_base);
            GA_KERNEL_CHECK();
        }
    }
    {
        StageTimer tm(ctx, "pairing_final");
        // gt on the host: the accumulators are overwritten in place (a lane reads its group before it writes it) and copied out
        Fe12<P>* d_gt = gt ? (o_dev ? (Fe12<P>*)gt : acc) : nullptr;
        hipLaunchKernelGGL((pairing_final_kernel<P>), dim3(capped_grid(n_groups, PAIRING_THREADS, PAIRING_MAX_BLOCKS)), dim3(PAIRING_THREADS), 0, st,
                           (const Fe12<P>*)acc, (uint32_t)n_groups, ok ? (o_dev ? ok : d_ok) : (uint8_t*)nullptr, d_gt, cnt);
        GA_KERNEL_CHECK();
    }
    if (ok) GA_CHECK(chunk_out(st, o_dev, ok, 0, n_groups, d_ok));
    if (gt) GA_CHECK(chunk_out(st, o_dev, (Fe12<P>*)gt, 0, n_groups, acc));
    PairingCounters h;
    GA_HIP_CHECK(hipMemcpyAsync(&h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
    GA_HIP_CHECK(hipStreamSynchronize(st));   // the one synchronisation of the call
    out2[0] = h.bad;
    out2[1] = h.bad ? (uint64_t)(uint32_t)~h.first_inv : UINT64_MAX;
    return GA_OK;
}

// what pairing_<curve>.hip instantiates
#define GA_INSTANTIATE_PAIRING(C) \
    template int pairing_run<C>(Ctx*, const void*, const void*, size_t, const uint64_t*, size_t, unsigned, uint8_t*, void*, uint64_t*, uint64_t);

}  // namespace ga

// plonk.Verify for `count` proofs under one key (backend/plonk/<curve>/verify.go:124-318): the per-proof scalar side on the device, and
// the driver that puts it between the calls the library already has -- check_points (verify.go:61-85), sparse_sums or the MSM, pairing.
// The challenges gamma, beta, alpha, zeta, v (kzg.FoldProof) and u (kzg.BatchVerifyMultiPoints) are inputs.
//
// Every Fr value is a Montgomery image below r in the packed representation (Fe<FrP>): the kernels are a few hundred products per
// proof beside 2 (9 + nb_bsb) scalar multiplications and two Miller loops, so they use the plain field and its out-of-line product
// (mul_val, one copy per field), not the 29-bit lazy layer.  The inverse of 0 is 0 (inv is the Fermat power), which is fr.Inverse's,
// BatchInvert's and Div's convention: zeta = w^k gives what verify.go computes.
//
//   plonk_vf_public_kernel    PI(zeta) (:136-188): the m = nb_public + nb_bsb terms x_i w^k_i / n (zeta^n - 1) / (zeta - w^k_i), k_i = i for
//                             the public inputs and nb_public + CommitmentConstraintIndexes[t] for the BSB22 hashes.  Grid over
//                             (proof, run of PLONK_VF_RUN = 8 terms): a lane inverts its run's denominators with ONE Fermat inversion
//                             (Montgomery's trick, zeros left out as BatchInvert leaves them) and writes the run's sum.
//   plonk_vf_rows_kernel      one lane per proof: zeta^n by log n squarings, zeta^(n+2), L_1(zeta), PI as the sum of the proof's runs, the
//                             relation constLin == ClaimedValues[0] (:206-223), the scalars of the linearised digest (:225-277), the
//                             fold in v (kzg.FoldProof) and the batching in u (kzg.BatchVerifyMultiPoints): the coefficient row
//                               G1 Ql Qr Qm Qo Qk S1 S2 S3 Qcp_0.. | L R O Z H0 H1 H2 W_zeta W_zeta_omega Bsb_0.. | -1, -u
//                             of  P = F - E G1 + zeta W_zeta + u (Z - zu G1 + w zeta W_zeta_omega),  Q = -(W_zeta + u W_zeta_omega).
//   plonk_vf_scale_kernel     combined mode: proof columns and the Q side times rho_j, written where the two MSMs read their scalars;
//   plonk_vf_openings_kernel  and W_zeta, W_zeta_omega of every proof side by side, the bases of Q;
//   plonk_vf_colsum_kernel    the key columns' weighted sums over the proofs: a lane per (column, slice of 256 proofs), then a lane per
//                             column over the slices.
// What bounds them: the public kernel one 255-step Fermat power per 8 terms (about 50 products per term), the rows kernel one per proof;
// both are compute-bound on the integer pipe and read 32 B per operand once.
#pragma once
#include <vector>

#include "hostops.hip.h"    // host_msm
#include "ntt.hip.h"        // Domain
#include "vec_call.hip.h"   // StreamDrain, capped_grid, chunk_out

namespace ga {

constexpr unsigned PLONK_VF_THREADS = 256;
constexpr unsigned PLONK_VF_MAX_BLOCKS = 1024;   // workgroups of a launch (grid-stride beyond): four per CU
constexpr uint32_t PLONK_VF_RUN = 8;             // terms of PI per lane: one inversion for all of them
constexpr uint32_t PLONK_VF_SLICE = 256;         // proofs per lane of the first level of the column sums
constexpr uint32_t PLONK_VF_FIXED = 9;           // key columns before Qcp (G1 Ql Qr Qm Qo Qk S1 S2 S3) = proof columns before Bsb
constexpr uint32_t PLONK_VF_W_ZETA = 7;          // W_zeta, W_zeta_omega: proof columns 7 and 8

struct PlonkVfShape {
    uint32_t count, nb_bsb;
    uint32_t nseg;        // runs of PI terms per proof
    int logn;
    uint64_t nb_public;
};

template <class FrP>
GA_HD Fe<FrP> vf_mul(const Fe<FrP>& a, const Fe<FrP>& b) { return mul_val<FrP>(a, b); }

template <class FrP>
__global__ void __launch_bounds__(PLONK_VF_THREADS)
plonk_vf_public_kernel(const PlonkVfShape sh, const Fe<FrP> omega, const Fe<FrP> ninv, const uint32_t* __restrict__ chal, const uint32_t* __restrict__ pub,
                       const uint32_t* __restrict__ hashes, const uint64_t* __restrict__ bsb_k, uint32_t* __restrict__ part) {
    typedef Fe<FrP> F;
    const uint64_t m = sh.nb_public + sh.nb_bsb, total = (uint64_t)sh.count * sh.nseg;
    for (uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t j = id / sh.nseg, first = (id % sh.nseg) * PLONK_VF_RUN;
        const F zeta = load_pod<F>(chal + (j * 6 + 3) * 8);
        F zn = zeta;
#pragma unroll 1
        for (int k = 0; k < sh.logn; k++) zn = vf_mul(zn, zn);
        const F c = vf_mul(sub(zn, fe_one<FrP>()), ninv);   // (zeta^n - 1) / n
        // forward: w^k_i and the products of the non-zero denominators before each term
        F w[PLONK_VF_RUN], pre[PLONK_VF_RUN];
        F acc = fe_one<FrP>(), wk = fe_zero<FrP>();
        uint64_t prev = 0;
#pragma unroll
        for (uint32_t k = 0; k < PLONK_VF_RUN; k++) {
            const uint64_t i = first + k;
            if (i < m) {
                const uint64_t e = i < sh.nb_public ? i : bsb_k[i - sh.nb_public];
                wk = (k > 0 && e == prev + 1) ? vf_mul(wk, omega) : pow_u64(omega, e);
                prev = e;
                w[k] = wk;
                pre[k] = acc;
                const F den = sub(zeta, wk);
                if (!is_zero(den)) acc = vf_mul(acc, den);
            }
        }
        // backward: 1 / den_k = (1 / product so far) * pre_k; a zero denominator contributes nothing (its inverse is 0)
        F ia = inv(acc), sum = fe_zero<FrP>();
#pragma unroll
        for (int k = (int)PLONK_VF_RUN - 1; k >= 0; k--) {
            const uint64_t i = first + k;
            if (i < m) {
                const F den = sub(zeta, w[k]);
                if (!is_zero(den)) {
                    const F x = load_pod<F>(i < sh.nb_public ? pub + (j * sh.nb_public + i) * 8 : hashes + (j * sh.nb_bsb + (i - sh.nb_public)) * 8);
                    sum = add(sum, vf_mul(vf_mul(x, w[k]), vf_mul(c, vf_mul(ia, pre[k]))));
                    ia = vf_mul(ia, den);
                }
            }
        }
        store_pod(part + id * 8, sum);
    }
}

// evals: [count][7 + nb_bsb], chal: [count][6], part: [count][nseg]; rows: [count][2 (9 + nb_bsb) + 2]
template <class FrP>
__global__ void __launch_bounds__(PLONK_VF_THREADS)
plonk_vf_rows_kernel(const PlonkVfShape sh, const Fe<FrP> omega, const Fe<FrP> ninv, const Fe<FrP> shift, const uint32_t* __restrict__ evals,
                     const uint32_t* __restrict__ chal, const uint32_t* __restrict__ part, uint32_t* __restrict__ rows, uint8_t* __restrict__ rel_ok) {
    typedef Fe<FrP> F;
    const uint32_t nb = sh.nb_bsb, np = PLONK_VF_FIXED + nb, ne = 7 + nb;
    const uint64_t W = 2 * (uint64_t)np + 2;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < sh.count; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t* e = evals + j * ne * 8;
        const uint32_t* ch = chal + j * 6 * 8;
        uint32_t* vkc = rows + j * W * 8;          // the key columns
        uint32_t* prc = vkc + (uint64_t)np * 8;    // the proof columns
        const F gamma = load_pod<F>(ch), beta = load_pod<F>(ch + 8), alpha = load_pod<F>(ch + 16), zeta = load_pod<F>(ch + 24);
        const F v = load_pod<F>(ch + 32), u = load_pod<F>(ch + 40);
        const F cv0 = load_pod<F>(e), l = load_pod<F>(e + 8), r = load_pod<F>(e + 16), o = load_pod<F>(e + 24);
        const F s1 = load_pod<F>(e + 32), s2 = load_pod<F>(e + 40), zu = load_pod<F>(e + (uint64_t)(6 + nb) * 8);
        const F one = fe_one<FrP>();

        F zn = zeta;
#pragma unroll 1
        for (int k = 0; k < sh.logn; k++) zn = vf_mul(zn, zn);
        const F zh = sub(zn, one);                                         // zeta^n - 1
        const F zn2 = vf_mul(zn, vf_mul(zeta, zeta));                      // zeta^(n+2)
        const F l1 = vf_mul(vf_mul(zh, ninv), inv(sub(zeta, one)));        // L_1(zeta)
        F pi = fe_zero<FrP>();
#pragma unroll 1
        for (uint32_t s = 0; s < sh.nseg; s++) pi = add(pi, load_pod<F>(part + (j * sh.nseg + s) * 8));

        // the algebraic relation (:206-223)
        const F a2l1 = vf_mul(vf_mul(l1, alpha), alpha);
        const F ab = vf_mul(add(add(vf_mul(beta, s1), gamma), l), add(add(vf_mul(beta, s2), gamma), r));
        const F abz = vf_mul(vf_mul(ab, alpha), zu);                       // alpha (l + beta s1 + gamma)(r + beta s2 + gamma) z(w zeta)
        const F const_lin = neg(add(sub(vf_mul(abz, add(o, gamma)), a2l1), pi));
        rel_ok[j] = eq(const_lin, cv0) ? 1 : 0;

        // the scalars of the linearised digest (:225-277)
        const F s1c = vf_mul(abz, beta);
        const F bz = vf_mul(beta, zeta), bzs = vf_mul(bz, shift);
        F t = vf_mul(add(add(bz, gamma), l), add(add(bzs, gamma), r));
        t = vf_mul(t, add(add(vf_mul(bzs, shift), o), gamma));
        const F coeff_z = sub(a2l1, vf_mul(t, alpha));
        const F h1 = vf_mul(zn2, zh);

        // E = sum_k v^k ClaimedValues[k] and the powers of v on their columns (kzg.FoldProof)
        F E = cv0, vp = one;
#pragma unroll 1
        for (uint32_t k = 1; k < 6 + nb; k++) {
            vp = vf_mul(vp, v);
            E = add(E, vf_mul(vp, load_pod<F>(e + (uint64_t)k * 8)));
            uint32_t* dst = k <= 3 ? prc + (k - 1) * 8 : k <= 5 ? vkc + (k + 2) * 8 : vkc + (uint64_t)(PLONK_VF_FIXED + k - 6) * 8;   // L R O | S1 S2 | Qcp
            store_pod(dst, vp);
        }
        store_pod(vkc, neg(add(E, vf_mul(u, zu))));   // G1
        store_pod(vkc + 8, l);                         // Ql
        store_pod(vkc + 16, r);                        // Qr
        store_pod(vkc + 24, vf_mul(l, r));             // Qm
        store_pod(vkc + 32, o);                        // Qo
        store_pod(vkc + 40, one);                      // Qk
        store_pod(vkc + 64, s1c);                      // S3
        store_pod(prc + 24, add(coeff_z, u));          // Z: the digest's and the second opening's
        store_pod(prc + 32, neg(zh));                  // H0
        store_pod(prc + 40, neg(h1));                  // H1
        store_pod(prc + 48, neg(vf_mul(zn2, h1)));     // H2
        store_pod(prc + 56, zeta);                     // W_zeta
        store_pod(prc + 64, vf_mul(u, vf_mul(omega, zeta)));   // W_zeta_omega
#pragma unroll 1
        for (uint32_t k = 0; k < nb; k++) store_pod(prc + (uint64_t)(PLONK_VF_FIXED + k) * 8, load_pod<F>(e + (uint64_t)(6 + k) * 8));   // Bsb_k: Qcp_k(zeta)
        store_pod(prc + (uint64_t)np * 8, neg(one));
        store_pod(prc + (uint64_t)np * 8 + 8, neg(u));
    }
}

// combined mode: scal[np + j np + c] = rho_j row_j[np + c] (c < np), qscal[2 j + c] = rho_j row_j[2 np + c] (c < 2)
template <class FrP>
__global__ void __launch_bounds__(PLONK_VF_THREADS)
plonk_vf_scale_kernel(uint32_t count, uint32_t np, const uint32_t* __restrict__ rows, const uint32_t* __restrict__ rho, uint32_t* __restrict__ scal,
                      uint32_t* __restrict__ qscal) {
    typedef Fe<FrP> F;
    const uint64_t per = (uint64_t)np + 2, total = count * per, W = 2 * (uint64_t)np + 2;
    for (uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t j = id / per, c = id % per;
        const F x = vf_mul(load_pod<F>(rho + j * 8), load_pod<F>(rows + (j * W + np + c) * 8));
        store_pod(c < np ? scal + (np + j * np + c) * 8 : qscal + (2 * j + (c - np)) * 8, x);
    }
}

// w[2 j + c] = proof j's opening proof c (W_zeta, W_zeta_omega) out of its np points
template <class A>
__global__ void __launch_bounds__(PLONK_VF_THREADS)
plonk_vf_openings_kernel(uint32_t count, uint32_t np, const A* __restrict__ proof_points, A* __restrict__ w) {
    for (uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; id < 2 * (uint64_t)count; id += (uint64_t)gridDim.x * blockDim.x)
        store_pod(&w[id], load_pod<A>(&proof_points[(id / 2) * np + PLONK_VF_W_ZETA + (id & 1)]));
}

// out[s][c] = sum over the PLONK_VF_SLICE items of slice s of (rho_j *) in[j][c], c < np: level 0 reads the rows (stride W) and weighs
// them, level 1 adds the slices' sums (stride np, rho == nullptr); n_slices = 1 leaves the sums in out[0]
template <class FrP>
__global__ void __launch_bounds__(PLONK_VF_THREADS)
plonk_vf_colsum_kernel(uint64_t n, uint32_t np, uint64_t stride, uint64_t slice, const uint32_t* __restrict__ in, const uint32_t* __restrict__ rho,
                       uint32_t* __restrict__ out) {
    typedef Fe<FrP> F;
    const uint64_t n_slices = (n + slice - 1) / slice, total = n_slices * np;
    for (uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t s = id / np, c = id % np, end = (s + 1) * slice < n ? (s + 1) * slice : n;
        F acc = fe_zero<FrP>();
#pragma unroll 1
        for (uint64_t j = s * slice; j < end; j++) {
            const F x = load_pod<F>(in + (j * stride + c) * 8);
            acc = add(acc, rho ? vf_mul(load_pod<F>(rho + j * 8), x) : x);
        }
        store_pod(out + id * 8, acc);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct PlonkVk {
    Domain* d0 = nullptr;
    uint64_t nb_public = 0;
    uint32_t nb_bsb = 0;
    void* d_points = nullptr;       // [9 + nb_bsb] G1Affine: G1 Ql Qr Qm Qo Qk S1 S2 S3 Qcp_0..
    uint64_t* d_bsb_k = nullptr;    // [nb_bsb] nb_public + CommitmentConstraintIndexes[t]
    std::vector<uint8_t> g2;        // vk.Kzg.G2[0], G2[1]: two G2Affine images
    uint32_t np() const { return PLONK_VF_FIXED + nb_bsb; }
    uint32_t width() const { return 2 * np() + 2; }
    uint32_t nseg() const { return (uint32_t)((nb_public + nb_bsb + PLONK_VF_RUN - 1) / PLONK_VF_RUN); }
};

// (plonk_vk_delete and plonk_vk_domain0, the accessors abi.hip uses, are in ntt_domain.hip)
inline void plonk_vk_free(PlonkVk* vk) {
    if (!vk) return;
    if (vk->d_points) hipFree(vk->d_points);
    if (vk->d_bsb_k) hipFree(vk->d_bsb_k);
    delete vk;
}

template <class C>
int plonk_vk_new(Domain* d0, const ga_plonk_vk_in* in, PlonkVk** out) {
    typedef Affine<Fe<typename C::FpP>> A1;
    typedef Affine<Fe2<typename C::FpP>> A2;
    const char* me = current_entry();
    if (in->nb_bsb > (uint32_t)PLONK_MAX_BSB) {
        set_error("%s: nb_bsb = %u above %d", me, in->nb_bsb, PLONK_MAX_BSB);
        return GA_ERR_INVALID;
    }
    if (!in->ql || !in->qr || !in->qm || !in->qo || !in->qk || !in->s1 || !in->s2 || !in->s3 || !in->kzg_g1 || !in->kzg_g2 ||
        (in->nb_bsb && (!in->qcp || !in->commitment_constraint_indexes))) {
        set_error("%s: null argument", me);
        return GA_ERR_INVALID;
    }
    if (in->nb_public > d0->n || in->nb_bsb > d0->n - in->nb_public) {
        set_error("%s: nb_public + nb_bsb = %llu + %u above the domain's size %llu", me, (unsigned long long)in->nb_public, in->nb_bsb, (unsigned long long)d0->n);
        return GA_ERR_INVALID;
    }
    std::vector<uint64_t> ks(in->nb_bsb ? in->nb_bsb : 1, 0);
    for (uint32_t t = 0; t < in->nb_bsb; t++) {
        const uint64_t cci = in->commitment_constraint_indexes[t];
        if (cci >= d0->n - in->nb_public) {
            set_error("%s: commitment_constraint_indexes[%u] = %llu puts its term at or beyond the domain's size %llu (nb_public = %llu)", me, t,
                      (unsigned long long)cci, (unsigned long long)d0->n, (unsigned long long)in->nb_public);
            return GA_ERR_INVALID;
        }
        ks[t] = in->nb_public + cci;
    }
    PlonkVk* vk = new PlonkVk;
    vk->d0 = d0;
    vk->nb_public = in->nb_public;
    vk->nb_bsb = in->nb_bsb;
    vk->g2.assign((const uint8_t*)in->kzg_g2, (const uint8_t*)in->kzg_g2 + 2 * sizeof(A2));
    std::vector<A1> pts(vk->np());
    const void* fixed[PLONK_VF_FIXED] = {in->kzg_g1, in->ql, in->qr, in->qm, in->qo, in->qk, in->s1, in->s2, in->s3};
    for (uint32_t k = 0; k < PLONK_VF_FIXED; k++) memcpy(&pts[k], fixed[k], sizeof(A1));
    if (in->nb_bsb) memcpy(&pts[PLONK_VF_FIXED], in->qcp, in->nb_bsb * sizeof(A1));
    auto fail = [&](int rc) {
        plonk_vk_free(vk);
        return rc;
    };
    hipError_t e = device_malloc(&vk->d_points, pts.size() * sizeof(A1));
    if (e == hipSuccess) e = device_malloc(&vk->d_bsb_k, ks.size() * 8);
    if (e != hipSuccess) {
        set_error("%s: device_malloc failed: %s", me, device_malloc_error(e));
        return fail(GA_ERR_NOMEM);
    }
    if (hipMemcpy(vk->d_points, pts.data(), pts.size() * sizeof(A1), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(vk->d_bsb_k, ks.data(), ks.size() * 8, hipMemcpyHostToDevice) != hipSuccess) {
        set_error("%s: the upload of the key failed", me);
        return fail(GA_ERR_HIP);
    }
    *out = vk;
    return GA_OK;
}

// The four Fr operands of `count` proofs on the device: where the caller has them, or staged into the context's scratch.  reserve()
// before the first launch of the call (an allocation failure leaves nothing in flight), upload() on the stream.
struct PlonkVfOperands {
    const ga_plonk_proofs* p;
    bool on_device;
    uint64_t bytes[4];
    const void* host[4];
    const uint32_t* dev[4] = {nullptr, nullptr, nullptr, nullptr};   // evals, challenges, public inputs, hashes
    PlonkVfOperands(const PlonkVk* vk, const ga_plonk_proofs* pr, uint32_t count, bool dev_ptrs) : p(pr), on_device(dev_ptrs) {
        bytes[0] = (uint64_t)count * (7 + vk->nb_bsb) * 32;
        bytes[1] = (uint64_t)count * 6 * 32;
        bytes[2] = (uint64_t)count * vk->nb_public * 32;
        bytes[3] = (uint64_t)count * vk->nb_bsb * 32;
        host[0] = p->evals;
        host[1] = p->challenges;
        host[2] = p->public_inputs;
        host[3] = p->bsb_hashes;
    }
    bool complete() const {
        for (int k = 0; k < 4; k++)
            if (bytes[k] && !host[k]) return false;
        return p->points != nullptr;
    }
    int reserve(Ctx* ctx) {
        static const char* const keys[4] = {"plonk_vf_evals", "plonk_vf_challenges", "plonk_vf_public", "plonk_vf_hashes"};
        for (int k = 0; k < 4; k++) {
            if (on_device || !bytes[k]) dev[k] = (const uint32_t*)host[k];
            else GA_CHECK(ctx->scratch_get(keys[k], bytes[k], (void**)&dev[k]));
        }
        return GA_OK;
    }
    int upload(hipStream_t st) {
        if (on_device) return GA_OK;
        for (int k = 0; k < 4; k++)
            if (bytes[k]) GA_HIP_CHECK(hipMemcpyAsync((void*)dev[k], host[k], bytes[k], hipMemcpyHostToDevice, st));
        return GA_OK;
    }
};

template <class FrP>
inline PlonkVfShape plonk_vf_shape(const PlonkVk* vk, uint32_t count) {
    return PlonkVfShape{count, vk->nb_bsb, vk->nseg(), vk->d0->logn, vk->nb_public};
}

// launches only: the rows and relation_ok of `count` proofs; part: count * nseg elements of scratch
template <class C>
int plonk_vf_launch_rows(Ctx* ctx, hipStream_t st, const PlonkVk* vk, uint32_t count, const PlonkVfOperands& ops, uint32_t* part, uint32_t* rows, uint8_t* rel) {
    typedef typename C::FrP FrP;
    typedef Fe<FrP> F;
    const PlonkVfShape sh = plonk_vf_shape<FrP>(vk, count);
    F omega, ninv;
    memcpy(&omega, vk->d0->w, 32);
    memcpy(&ninv, vk->d0->ninv_mont, 32);
    const F shift = fe_const<FrP>(FrP::GEN);   // vk.CosetShift: the multiplicative generator fft.NewDomain takes
    if (sh.nseg) {
        StageTimer tm(ctx, "plonk_vf_public");
        hipLaunchKernelGGL((plonk_vf_public_kernel<FrP>), dim3(capped_grid((uint64_t)count * sh.nseg, PLONK_VF_THREADS, PLONK_VF_MAX_BLOCKS)),
                           dim3(PLONK_VF_THREADS), 0, st, sh, omega, ninv, ops.dev[1], ops.dev[2], ops.dev[3], (const uint64_t*)vk->d_bsb_k, part);
        GA_KERNEL_CHECK();
    }
    StageTimer tm(ctx, "plonk_vf_rows");
    hipLaunchKernelGGL((plonk_vf_rows_kernel<FrP>), dim3(capped_grid(count, PLONK_VF_THREADS, PLONK_VF_MAX_BLOCKS)), dim3(PLONK_VF_THREADS), 0, st, sh, omega, ninv,
                       shift, ops.dev[0], ops.dev[1], (const uint32_t*)part, rows, rel);
    GA_KERNEL_CHECK();
    return GA_OK;
}

template <class C>
int plonk_verify_scalars_run(PlonkVk* vk, const ga_plonk_proofs* p, uint32_t count, bool on_device, void* rows_out, uint8_t* relation_ok) {
    Ctx* ctx = vk->d0->ctx;
    PlonkVfOperands ops(vk, p, count, on_device);
    if (!ops.complete()) {
        set_error("%s: null argument", current_entry());
        return GA_ERR_INVALID;
    }
    const uint64_t row_words = (uint64_t)count * vk->width() * 8;
    hipStream_t st = ctx->work_stream();
    uint32_t *part = nullptr, *d_rows = nullptr;
    uint8_t* d_rel = nullptr;
    GA_CHECK(ops.reserve(ctx));
    if (vk->nseg()) GA_CHECK(ctx->scratch_get("plonk_vf_partial", (uint64_t)count * vk->nseg() * 32, (void**)&part));
    if (!on_device) {
        GA_CHECK(ctx->scratch_get("plonk_vf_rows", row_words * 4, (void**)&d_rows));
        GA_CHECK(ctx->scratch_get("plonk_vf_relation", count, (void**)&d_rel));
    }
    StreamDrain drain{st};
    GA_CHECK(ops.upload(st));
    GA_CHECK(plonk_vf_launch_rows<C>(ctx, st, vk, count, ops, part, on_device ? (uint32_t*)rows_out : d_rows, on_device ? relation_ok : d_rel));
    GA_CHECK(chunk_out(st, on_device, (uint32_t*)rows_out, 0, row_words, d_rows));
    GA_CHECK(chunk_out(st, on_device, relation_ok, 0, count, d_rel));
    GA_HIP_CHECK(hipStreamSynchronize(st));   // the one synchronisation of the call
    return GA_OK;
}

template <class C>
int plonk_verify_run(PlonkVk* vk, const ga_plonk_proofs* p, uint32_t count, unsigned flags, const void* weights, uint8_t* ok, uint8_t* relation_ok,
                     uint64_t* out2, const PlonkVerifyKnobs& knobs) {
    typedef typename C::FrP FrP;
    typedef Fe<FrP> F;
    typedef Affine<Fe<typename C::FpP>> A1;
    typedef Affine<Fe2<typename C::FpP>> A2;
    Ctx* ctx = vk->d0->ctx;
    const bool on_device = (flags & GA_PLONK_ON_DEVICE) != 0, combined = (flags & GA_PLONK_VERIFY_COMBINED) != 0;
    const uint32_t np = vk->np(), W = vk->width();
    const uint64_t n_proof_pts = (uint64_t)count * np, n_pts = np + n_proof_pts;
    PlonkVfOperands ops(vk, p, count, on_device);
    if (!ops.complete()) {
        set_error("%s: null argument", current_entry());
        return GA_ERR_INVALID;
    }
    hipStream_t st = ctx->work_stream();

    // verify.go:61-85: a proof with a point off the curve or outside the subgroup is rejected; its terms never enter a sum
    std::vector<uint8_t> rejected(count, 0);
    if (!(flags & GA_PLONK_VERIFY_NO_POINT_CHECK)) {
        std::vector<uint8_t> status(n_proof_pts);
        uint64_t out4[4];
        GA_CHECK((check_points_run<C, GA_G1>(ctx, p->points, n_proof_pts, on_device ? GA_BASES_ON_DEVICE : 0u, status.data(), out4, knobs.check_naive,
                                             knobs.check_chunk)));
        if (out4[0] | out4[1])
            for (uint64_t i = 0; i < n_proof_pts; i++)
                if (status[i] != GA_POINT_OK) rejected[i / np] = 1;
    }

    // the rows: the scratch of this stage first, then the launches and the one synchronisation that brings rows and relations to the host
    std::vector<uint32_t> h_rows((uint64_t)count * W * 8);
    std::vector<uint8_t> h_rel(count);
    uint32_t *part = nullptr, *d_rows, *d_rho = nullptr, *d_scal = nullptr, *d_qscal = nullptr, *d_sl = nullptr;
    uint8_t* d_rel = nullptr;
    A1 *d_pts, *d_w = nullptr;
    const uint64_t n_slices = ((uint64_t)count + PLONK_VF_SLICE - 1) / PLONK_VF_SLICE;
    GA_CHECK(ops.reserve(ctx));
    if (vk->nseg()) GA_CHECK(ctx->scratch_get("plonk_vf_partial", (uint64_t)count * vk->nseg() * 32, (void**)&part));
    GA_CHECK(ctx->scratch_get("plonk_vf_rows", h_rows.size() * 4, (void**)&d_rows));
    if (!(on_device && relation_ok)) GA_CHECK(ctx->scratch_get("plonk_vf_relation", count, (void**)&d_rel));
    GA_CHECK(ctx->scratch_get("plonk_vf_points", n_pts * sizeof(A1), (void**)&d_pts));
    A1* d_pq = nullptr;
    A2* d_g2 = nullptr;
    std::vector<uint8_t> tiled;   // G2[0], G2[1] once per group
    if (!combined) {
        GA_CHECK(ctx->scratch_get("plonk_vf_pq", (uint64_t)count * 2 * sizeof(A1), (void**)&d_pq));
        GA_CHECK(ctx->scratch_get("plonk_vf_g2", (uint64_t)count * 2 * sizeof(A2), (void**)&d_g2));
        tiled.resize((uint64_t)count * 2 * sizeof(A2));
        for (uint32_t j = 0; j < count; j++) memcpy(&tiled[(uint64_t)j * 2 * sizeof(A2)], vk->g2.data(), 2 * sizeof(A2));
    } else {
        GA_CHECK(ctx->scratch_get("plonk_vf_weights", (uint64_t)count * 32, (void**)&d_rho));
        GA_CHECK(ctx->scratch_get("plonk_vf_scalars", n_pts * 32, (void**)&d_scal));
        GA_CHECK(ctx->scratch_get("plonk_vf_q_scalars", (uint64_t)count * 64, (void**)&d_qscal));
        GA_CHECK(ctx->scratch_get("plonk_vf_q_points", (uint64_t)count * 2 * sizeof(A1), (void**)&d_w));
        GA_CHECK(ctx->scratch_get("plonk_vf_slices", n_slices * np * 32, (void**)&d_sl));
    }
    uint8_t* rel_dev = (on_device && relation_ok) ? relation_ok : d_rel;
    {
        StreamDrain drain{st};
        GA_CHECK(ops.upload(st));
        GA_CHECK(plonk_vf_launch_rows<C>(ctx, st, vk, count, ops, part, d_rows, rel_dev));
        // [key points | proof points]: what the row sums and the MSM index
        GA_HIP_CHECK(hipMemcpyAsync(d_pts, vk->d_points, np * sizeof(A1), hipMemcpyDeviceToDevice, st));
        GA_HIP_CHECK(hipMemcpyAsync(d_pts + np, p->points, n_proof_pts * sizeof(A1), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        if (combined) {
            GA_HIP_CHECK(hipMemcpyAsync(d_rho, weights, (uint64_t)count * 32, hipMemcpyHostToDevice, st));
            StageTimer tm(ctx, "plonk_vf_combine");
            hipLaunchKernelGGL((plonk_vf_scale_kernel<FrP>), dim3(capped_grid((uint64_t)count * (np + 2), PLONK_VF_THREADS, PLONK_VF_MAX_BLOCKS)), dim3(PLONK_VF_THREADS),
                               0, st, count, np, (const uint32_t*)d_rows, (const uint32_t*)d_rho, d_scal, d_qscal);
            // the key columns: slices of the weighted rows, then the slices' sums into the first np scalars
            hipLaunchKernelGGL((plonk_vf_colsum_kernel<FrP>), dim3(capped_grid(n_slices * np, PLONK_VF_THREADS, PLONK_VF_MAX_BLOCKS)), dim3(PLONK_VF_THREADS), 0, st,
                               (uint64_t)count, np, (uint64_t)W, (uint64_t)PLONK_VF_SLICE, (const uint32_t*)d_rows, (const uint32_t*)d_rho, d_sl);
            hipLaunchKernelGGL((plonk_vf_colsum_kernel<FrP>), dim3(1), dim3(PLONK_VF_THREADS), 0, st, n_slices, np, (uint64_t)np, n_slices, (const uint32_t*)d_sl,
                               (const uint32_t*)nullptr, d_scal);
            GA_KERNEL_CHECK();
            // W_zeta, W_zeta_omega of every proof side by side: the bases of Q
            hipLaunchKernelGGL((plonk_vf_openings_kernel<A1>), dim3(capped_grid((uint64_t)count * 2, PLONK_VF_THREADS, PLONK_VF_MAX_BLOCKS)), dim3(PLONK_VF_THREADS), 0, st,
                               count, np, (const A1*)(d_pts + np), d_w);
            GA_KERNEL_CHECK();
        } else {
            GA_HIP_CHECK(hipMemcpyAsync(h_rows.data(), d_rows, h_rows.size() * 4, hipMemcpyDeviceToHost, st));
            GA_HIP_CHECK(hipMemcpyAsync(d_g2, tiled.data(), tiled.size(), hipMemcpyHostToDevice, st));
        }
        GA_HIP_CHECK(hipMemcpyAsync(h_rel.data(), rel_dev, count, hipMemcpyDeviceToHost, st));
        if (relation_ok && !on_device) GA_HIP_CHECK(hipMemcpyAsync(relation_ok, rel_dev, count, hipMemcpyDeviceToHost, st));
        GA_HIP_CHECK(hipStreamSynchronize(st));   // the one synchronisation of the scalar side
    }
    for (uint32_t j = 0; j < count; j++)
        if (!h_rel[j]) rejected[j] = 1;

    // A rejected proof's verdict comes out of the pairing like the others': its group is e(G1, G2[0]) e(O, G2[1]), which is not 1.
    const unsigned pair_out = on_device ? GA_RESULT_ON_DEVICE : 0u;
    const F one = fe_one<FrP>();
    if (combined) {
        bool any = false;
        for (uint32_t j = 0; j < count; j++) any |= rejected[j] != 0;
        A1 pq[2];
        memset(pq, 0, sizeof(pq));
        if (any)
            hipMemcpy(&pq[0], vk->d_points, sizeof(A1), hipMemcpyDeviceToHost);
        else {
            XYZZ<Fe<typename C::FpP>> sp, sq;
            GA_CHECK((host_msm<C, GA_G1>(ctx, d_pts, d_scal, n_pts, true, &sp)));
            GA_CHECK((host_msm<C, GA_G1>(ctx, d_w, d_qscal, (uint64_t)count * 2, true, &sq)));
            pq[0] = to_affine(sp);
            pq[1] = to_affine(sq);
        }
        return pairing_run<C>(ctx, pq, vk->g2.data(), 2, nullptr, 1, pair_out, ok, nullptr, out2, knobs.pairing_chunk);
    }

    // rows 2j, 2j + 1 of one sparse sum: P_j over [key points | proof j's points], Q_j over its two opening proofs
    std::vector<uint64_t> row_start(2 * (uint64_t)count + 1);
    std::vector<uint32_t> terms;
    terms.reserve((uint64_t)count * W * 2);
    const uint32_t cid_one = (uint32_t)((uint64_t)count * W);
    h_rows.resize(h_rows.size() + 8);
    memcpy(&h_rows[(uint64_t)cid_one * 8], &one, 32);
    row_start[0] = 0;
    for (uint32_t j = 0; j < count; j++) {
        const uint32_t c0 = j * W, p0 = np + j * np;
        if (rejected[j]) {
            terms.push_back(cid_one);
            terms.push_back(0);
            row_start[2 * j + 1] = row_start[2 * j + 2] = terms.size() / 2;
            continue;
        }
        for (uint32_t c = 0; c < np; c++) {
            terms.push_back(c0 + c);
            terms.push_back(c);
        }
        for (uint32_t c = 0; c < np; c++) {
            terms.push_back(c0 + np + c);
            terms.push_back(p0 + c);
        }
        row_start[2 * j + 1] = terms.size() / 2;
        for (uint32_t c = 0; c < 2; c++) {
            terms.push_back(c0 + 2 * np + c);
            terms.push_back(p0 + PLONK_VF_W_ZETA + c);
        }
        row_start[2 * j + 2] = terms.size() / 2;
    }
    GA_CHECK((sparse_sums_run<C, GA_G1>(ctx, d_pts, n_pts, row_start.data(), 2 * (size_t)count, terms.data(), h_rows.data(), (size_t)cid_one + 1,
                                        GA_BASES_ON_DEVICE | GA_RESULT_ON_DEVICE | GA_SCALARS_MONTGOMERY, d_pq, nullptr, knobs.sparse_chunk,
                                        knobs.sparse_segment, 0)));
    std::vector<uint64_t> group_start(count + 1);
    for (uint64_t g = 0; g <= count; g++) group_start[g] = 2 * g;
    return pairing_run<C>(ctx, d_pq, d_g2, 2 * (size_t)count, group_start.data(), count, GA_BASES_ON_DEVICE | pair_out, ok, nullptr, out2, knobs.pairing_chunk);
}

// what plonk_verify_<curve>.hip instantiates
#define GA_INSTANTIATE_PLONK_VERIFY(C)                                                                                      \
    template int plonk_vk_new<C>(Domain*, const ga_plonk_vk_in*, PlonkVk**);                                                \
    template int plonk_verify_scalars_run<C>(PlonkVk*, const ga_plonk_proofs*, uint32_t, bool, void*, uint8_t*);            \
    template int plonk_verify_run<C>(PlonkVk*, const ga_plonk_proofs*, uint32_t, unsigned, const void*, uint8_t*, uint8_t*, \
                                     uint64_t*, const PlonkVerifyKnobs&);

}  // namespace ga

// TEST INFRASTRUCTURE: one exported function that runs a single device primitive of the field layer (field.hip.h, field29.hip.h)
// or one point formula (msm_lazy.hip.h, msm_bucket.hip.h) on caller-supplied raw words, one thread per element, and returns the raw
// result.  The product headers are included unchanged; the kernels here load, call and store -- they reduce nothing themselves, so
// the tests see exactly what the product function left in its registers (tests/test_field_boundaries*.py, tests/field_cases.py).
// Built twice: by hipcc for gfx950 (gnark_amd/csrc/Makefile, target ../../tests/probe/libga_probe.so) and by g++ against the
// functional emulation (tests/probe/build_probe_emu.sh).  Never part of libgnark_amd.so.
#include "field.hip.h"
#include "field29.hip.h"
#include "ec.hip.h"
#include "msm_lazy.hip.h"
#include "msm_bucket.hip.h"

using namespace ga;

namespace {

// op codes (tests/field_cases.py keeps the same table)
enum {
    // packed Fe<P>: N words per operand
    OP_ADD = 0, OP_SUB, OP_NEG, OP_DBL, OP_MUL, OP_SQR, OP_INV, OP_FROM_MONT, OP_TO_MONT, OP_MUL_SMALL,
    // conversions
    OP_F29_FROM_MEM = 10, OP_F29_UNPACK, OP_F29_HAT_PACKED, OP_F29_TO_MEM, OP_F29_PACK_CANONICAL, OP_F29_PACK_HAT,
    // lazy F29<P>: NL raw limbs per operand
    OP_F29_NORMALIZE = 20, OP_F29_ADD, OP_F29_ADD_RAW, OP_F29_SUB, OP_F29_SUB_RAW, OP_F29_SUB_WIDE, OP_F29_MUL, OP_F29_SQR,
    OP_F29_MUL_SUB, OP_F29_PARTIAL_REDUCE, OP_F29_REDUCE_3P, OP_F29_IS_ZERO_MOD_P, OP_F29_INV,
    // F29x2<P>: c0 | c1, NL limbs each (base fields with an Fp2 only)
    OP_F29X2_MUL = 40, OP_F29X2_SQR, OP_F29X2_MUL_SUB, OP_F29X2_INV,
    // point formulas over Fe<Fp> (50..) and Fe2<Fp> (60..): coordinates of Lazy<F>::NW words, k = number of chained applications
    OP_PT_ADD29 = 50, OP_PT_DBL29, OP_PT_MADD29, OP_PT_MDBL29, OP_PT_MADD29_COMPLETE,
    OP_PT2_BASE = 60,
    // the signed-digit recoding of a scalar (msm_sort.hip.h DigitWalk), scalar fields only: 8 words | mont -> (key, value) x 64 windows
    OP_DIGIT_WALK = 70,
};
constexpr int MAX_CHAIN = 64;
constexpr int DIGIT_WINDOWS = 64;   // every window of a 256-bit scalar for c >= 4

// HasG1: a base field, the G1 point formulas run over Fe<P>.  HasFp2: Fe2<P>, F29x2<P> and P::FP2Z_K exist (not for BLS12-377, whose
// Fp2 would be u^2 + 5: Fe2 over it does not compile).  A scalar field has neither and gets the digit recoding instead.
template <class P> struct HasG1 { static constexpr bool value = false; };
template <> struct HasG1<BN254_Fp> { static constexpr bool value = true; };
template <> struct HasG1<BLS12_381_Fp> { static constexpr bool value = true; };
template <> struct HasG1<BLS12_377_Fp> { static constexpr bool value = true; };
template <class P> struct HasFp2 { static constexpr bool value = false; };
template <> struct HasFp2<BN254_Fp> { static constexpr bool value = true; };
template <> struct HasFp2<BLS12_381_Fp> { static constexpr bool value = true; };

template <class P>
__device__ __forceinline__ Fe<P> ld_fe(const uint32_t* p) {
    Fe<P> r;
#pragma unroll
    for (int i = 0; i < P::N; i++) r.l[i] = p[i];
    return r;
}
template <class P>
__device__ __forceinline__ void st(uint32_t* p, const Fe<P>& a) {
#pragma unroll
    for (int i = 0; i < P::N; i++) p[i] = a.l[i];
}
template <class P>
__device__ __forceinline__ F29<P> ld_l(const uint32_t* p) {
    F29<P> r;
#pragma unroll
    for (int i = 0; i < Radix<P>::NL; i++) r.l[i] = p[i];
    return r;
}
template <class P>
__device__ __forceinline__ void st(uint32_t* p, const F29<P>& a) {
#pragma unroll
    for (int i = 0; i < Radix<P>::NL; i++) p[i] = a.l[i];
}
template <class P>
__device__ __forceinline__ F29x2<P> ld_l2(const uint32_t* p) { return {ld_l<P>(p), ld_l<P>(p + Radix<P>::NL)}; }
template <class P>
__device__ __forceinline__ void st(uint32_t* p, const F29x2<P>& a) {
    st(p, a.c0);
    st(p + Radix<P>::NL, a.c1);
}
// a lazy coordinate of either field type through the uniform view the kernels use
template <class F>
__device__ __forceinline__ typename Lazy<F>::T ld_c(const uint32_t* p) {
    typename Lazy<F>::T r;
#pragma unroll
    for (int i = 0; i < Lazy<F>::NW; i++) Lazy<F>::set_word(r, i, p[i]);
    return r;
}
template <class F>
__device__ __forceinline__ void st_c(uint32_t* p, const typename Lazy<F>::T& v) {
#pragma unroll
    for (int i = 0; i < Lazy<F>::NW; i++) p[i] = Lazy<F>::word(v, i);
}

// ---- field primitives: words in / words out per element -------------------------------------------------------------------------
template <class P, int OP>
struct Shape {
    static constexpr int N = P::N, NL = Radix<P>::NL;
    static constexpr int IN = OP == OP_ADD || OP == OP_SUB || OP == OP_MUL ? 2 * N
                            : OP < 10 ? N
                            : OP == OP_F29_FROM_MEM || OP == OP_F29_UNPACK || OP == OP_F29_HAT_PACKED ? N
                            : OP < 20 ? NL
                            : OP == OP_F29_ADD || OP == OP_F29_ADD_RAW || OP == OP_F29_SUB || OP == OP_F29_SUB_RAW || OP == OP_F29_SUB_WIDE || OP == OP_F29_MUL ? 2 * NL
                            : OP == OP_F29_MUL_SUB ? 4 * NL
                            : OP < 40 ? NL
                            : OP == OP_F29X2_MUL ? 4 * NL
                            : OP == OP_F29X2_MUL_SUB ? 8 * NL
                            : 2 * NL;
    static constexpr int OUT = OP < 10 ? N
                             : OP == OP_F29_FROM_MEM || OP == OP_F29_UNPACK ? NL
                             : OP < 20 ? N
                             : OP == OP_F29_IS_ZERO_MOD_P ? 1
                             : OP < 40 ? NL
                             : 2 * NL;
};

template <class P, int OP, int K>
__device__ __forceinline__ void run_op(const uint32_t* in, uint32_t* out, int k) {
    constexpr int N = P::N, NL = Radix<P>::NL;
    if constexpr (OP == OP_ADD) st(out, add(ld_fe<P>(in), ld_fe<P>(in + N)));
    else if constexpr (OP == OP_SUB) st(out, sub(ld_fe<P>(in), ld_fe<P>(in + N)));
    else if constexpr (OP == OP_NEG) st(out, neg(ld_fe<P>(in)));
    else if constexpr (OP == OP_DBL) st(out, dbl(ld_fe<P>(in)));
    else if constexpr (OP == OP_MUL) st(out, mul_body(ld_fe<P>(in), ld_fe<P>(in + N)));
    else if constexpr (OP == OP_SQR) st(out, sqr(ld_fe<P>(in)));
    else if constexpr (OP == OP_INV) st(out, inv(ld_fe<P>(in)));
    else if constexpr (OP == OP_FROM_MONT) st(out, from_mont(ld_fe<P>(in)));
    else if constexpr (OP == OP_TO_MONT) st(out, to_mont(ld_fe<P>(in)));
    else if constexpr (OP == OP_MUL_SMALL) st(out, mul_small(ld_fe<P>(in), (uint32_t)k));
    else if constexpr (OP == OP_F29_FROM_MEM) st(out, f29_from_mem(ld_fe<P>(in)));
    else if constexpr (OP == OP_F29_UNPACK) st(out, f29_unpack(ld_fe<P>(in)));
    else if constexpr (OP == OP_F29_HAT_PACKED) st(out, f29_hat_packed(ld_fe<P>(in)));
    else if constexpr (OP == OP_F29_TO_MEM) st(out, f29_to_mem(ld_l<P>(in)));
    else if constexpr (OP == OP_F29_PACK_CANONICAL) st(out, f29_pack_canonical(ld_l<P>(in)));
    else if constexpr (OP == OP_F29_PACK_HAT) st(out, f29_pack_hat(ld_l<P>(in)));
    else if constexpr (OP == OP_F29_NORMALIZE) {
        F29<P> a = ld_l<P>(in);
        f29_normalize(a);
        st(out, a);
    }
    else if constexpr (OP == OP_F29_ADD) st(out, f29_add(ld_l<P>(in), ld_l<P>(in + NL)));
    else if constexpr (OP == OP_F29_ADD_RAW) st(out, f29_add_raw(ld_l<P>(in), ld_l<P>(in + NL)));
    else if constexpr (OP == OP_F29_SUB) st(out, f29_sub<K>(ld_l<P>(in), ld_l<P>(in + NL)));
    else if constexpr (OP == OP_F29_SUB_RAW) st(out, f29_sub_raw<K>(ld_l<P>(in), ld_l<P>(in + NL)));
    else if constexpr (OP == OP_F29_SUB_WIDE) st(out, f29_sub_wide<K, K>(ld_l<P>(in), ld_l<P>(in + NL)));
    else if constexpr (OP == OP_F29_MUL) st(out, f29_mul(ld_l<P>(in), ld_l<P>(in + NL)));
    else if constexpr (OP == OP_F29_SQR) st(out, f29_sqr(ld_l<P>(in)));
    else if constexpr (OP == OP_F29_MUL_SUB) st(out, f29_mul_sub<K>(ld_l<P>(in), ld_l<P>(in + NL), ld_l<P>(in + 2 * NL), ld_l<P>(in + 3 * NL)));
    else if constexpr (OP == OP_F29_PARTIAL_REDUCE) st(out, f29_partial_reduce(ld_l<P>(in)));
    else if constexpr (OP == OP_F29_REDUCE_3P) st(out, f29_reduce_3p(ld_l<P>(in)));
    else if constexpr (OP == OP_F29_IS_ZERO_MOD_P) out[0] = f29_is_zero_mod_p(ld_l<P>(in)) ? 1u : 0u;
    else if constexpr (OP == OP_F29_INV) st(out, f29_inv(ld_l<P>(in)));
    else if constexpr (OP == OP_F29X2_MUL) st(out, f29_mul(ld_l2<P>(in), ld_l2<P>(in + 2 * NL)));
    else if constexpr (OP == OP_F29X2_SQR) st(out, f29_sqr(ld_l2<P>(in)));
    else if constexpr (OP == OP_F29X2_MUL_SUB)
        st(out, f29_mul_sub<K>(ld_l2<P>(in), ld_l2<P>(in + 2 * NL), ld_l2<P>(in + 4 * NL), ld_l2<P>(in + 6 * NL)));
    else if constexpr (OP == OP_F29X2_INV) st(out, f29_inv(ld_l2<P>(in)));
}

template <class P, int OP, int K>
__global__ void __launch_bounds__(64) probe_kernel(const uint32_t* in, size_t n, uint32_t* out, int k) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    run_op<P, OP, K>(in + i * Shape<P, OP>::IN, out + i * Shape<P, OP>::OUT, k);
}

// ---- point formulas -------------------------------------------------------------------------------------------------------------
// general points in registers: a (4 coordinates) | b (4 coordinates, add29 only) -> a after k applications
template <class F, int OP>
__global__ void __launch_bounds__(64) probe_lazy4_kernel(const uint32_t* in, size_t n, uint32_t* out, int k) {
    constexpr int NW = Lazy<F>::NW, IN = OP == OP_PT_ADD29 ? 8 * NW : 4 * NW;
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint32_t* p = in + i * IN;
    Lazy4<F> a{ld_c<F>(p), ld_c<F>(p + NW), ld_c<F>(p + 2 * NW), ld_c<F>(p + 3 * NW)};
    if constexpr (OP == OP_PT_ADD29) {
        const Lazy4<F> b{ld_c<F>(p + 4 * NW), ld_c<F>(p + 5 * NW), ld_c<F>(p + 6 * NW), ld_c<F>(p + 7 * NW)};
        for (int s = 0; s < k; s++) add29<F>(a, b);
    } else {
        for (int s = 0; s < k; s++) dbl29<F>(a);
    }
    uint32_t* o = out + i * 4 * NW;
    st_c<F>(o, a.x);
    st_c<F>(o + NW, a.y);
    st_c<F>(o + 2 * NW, a.zz);
    st_c<F>(o + 3 * NW, a.zzz);
}

// the bucket loop's accumulator in LDS, laid out and launched as msm_accumulate29_kernel does: accumulator (4 coordinates; not
// mdbl29) | qx | qy -> accumulator after k applications (| the boolean of madd29_complete)
template <class F, int OP>
__global__ void __launch_bounds__(Table29<F>::THREADS) probe_acc_kernel(const uint32_t* in, size_t n, uint32_t* out, int k) {
    typedef typename Lazy<F>::Params P;
    constexpr int NW = Lazy<F>::NW, THREADS = Table29<F>::THREADS;
    constexpr int IN = OP == OP_PT_MDBL29 ? 2 * NW : 6 * NW, OUT = OP == OP_PT_MADD29_COMPLETE ? 4 * NW + 1 : 4 * NW;
    __shared__ uint32_t lds[4 * NW * THREADS];
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t* p = in + i * IN;
    LdsAcc29<F> A(lds + threadIdx.x);
    uint32_t ok = 1;
    if constexpr (OP == OP_PT_MDBL29) {
        mdbl29<F>(A, ld_c<F>(p), ld_c<F>(p + NW));
    } else {
        for (int f = 0; f < 4; f++) A.put(f, ld_c<F>(p + f * NW));
        const typename Lazy<F>::T qx = ld_c<F>(p + 4 * NW), qy = ld_c<F>(p + 5 * NW);
        for (int s = 0; s < k && ok; s++) {
            if constexpr (OP == OP_PT_MADD29) madd29<P>(A, qx, qy);
            else ok = madd29_complete<F>(A, qx, qy) ? 1u : 0u;
        }
    }
    uint32_t* o = out + i * OUT;
    for (int f = 0; f < 4; f++) st_c<F>(o + f * NW, A.get(f));
    if constexpr (OP == OP_PT_MADD29_COMPLETE) o[4 * NW] = ok;
}

// DigitWalk as msm_digits_kernel drives it for raw bases (one bucket set per window, win_lo = 0, key_base = 0, skip = ~0), element 0
template <class P>
__global__ void __launch_bounds__(64) probe_digits_kernel(const uint32_t* in, size_t n, uint32_t* out, int c) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    DigitWalk<P> D;
    D.set(ld_fe<P>(in + i * 9), (int)in[i * 9 + 8]);
    for (int w = 0; w < DIGIT_WINDOWS; w++) {
        uint32_t key, val;
        D.next(c, w, 0, n, 0, 0, 0u, 0xFFFFFFFFu, key, val);
        out[(i * DIGIT_WINDOWS + w) * 2] = key;
        out[(i * DIGIT_WINDOWS + w) * 2 + 1] = val;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
enum { PROBE_OK = 0, PROBE_BAD_ARGS = 1, PROBE_HIP_ERROR = 2 };
typedef void (*Kernel)(const uint32_t*, size_t, uint32_t*, int);

int launch(Kernel kern, unsigned threads, int want_in, int want_out, int k, const uint32_t* in, size_t n, size_t in_words, uint32_t* out,
           size_t out_words) {
    if ((size_t)want_in != in_words || (size_t)want_out != out_words || n > (1u << 20) || (n && (!in || !out))) return PROBE_BAD_ARGS;
    if (n == 0) return PROBE_OK;
    uint32_t *d_in = nullptr, *d_out = nullptr;
    int rc = PROBE_HIP_ERROR;
    if (hipMalloc((void**)&d_in, n * in_words * 4) == hipSuccess && hipMalloc((void**)&d_out, n * out_words * 4) == hipSuccess &&
        hipMemcpy(d_in, in, n * in_words * 4, hipMemcpyHostToDevice) == hipSuccess) {
        hipLaunchKernelGGL(kern, dim3((unsigned)((n + threads - 1) / threads)), dim3(threads), 0, (hipStream_t)0, (const uint32_t*)d_in, n, d_out, k);
        if (hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
            hipMemcpy(out, d_out, n * out_words * 4, hipMemcpyDeviceToHost) == hipSuccess)
            rc = PROBE_OK;
    }
    if (d_in) hipFree(d_in);
    if (d_out) hipFree(d_out);
    return rc;
}

#define GA_PROBE_ARGS in, n, in_words, out, out_words
#define GA_PROBE_FIELD_OP(OP, K) \
    return launch(probe_kernel<P, OP, K>, 64, Shape<P, OP>::IN, Shape<P, OP>::OUT, k, GA_PROBE_ARGS)

template <class F>
int run_point(int op, int k, const uint32_t* in, size_t n, size_t in_words, uint32_t* out, size_t out_words) {
    constexpr int NW = Lazy<F>::NW, AT = Table29<F>::THREADS;
    if (k < 1 || k > MAX_CHAIN) return PROBE_BAD_ARGS;
    switch (op) {
    case OP_PT_ADD29: return launch(probe_lazy4_kernel<F, OP_PT_ADD29>, 64, 8 * NW, 4 * NW, k, GA_PROBE_ARGS);
    case OP_PT_DBL29: return launch(probe_lazy4_kernel<F, OP_PT_DBL29>, 64, 4 * NW, 4 * NW, k, GA_PROBE_ARGS);
    case OP_PT_MADD29: return launch(probe_acc_kernel<F, OP_PT_MADD29>, AT, 6 * NW, 4 * NW, k, GA_PROBE_ARGS);
    case OP_PT_MDBL29: return launch(probe_acc_kernel<F, OP_PT_MDBL29>, AT, 2 * NW, 4 * NW, k, GA_PROBE_ARGS);
    case OP_PT_MADD29_COMPLETE: return launch(probe_acc_kernel<F, OP_PT_MADD29_COMPLETE>, AT, 6 * NW, 4 * NW + 1, k, GA_PROBE_ARGS);
    }
    return PROBE_BAD_ARGS;
}

template <class P>
int run_field(int op, int k, const uint32_t* in, size_t n, size_t in_words, uint32_t* out, size_t out_words) {
    switch (op) {
    case OP_ADD: GA_PROBE_FIELD_OP(OP_ADD, 0);
    case OP_SUB: GA_PROBE_FIELD_OP(OP_SUB, 0);
    case OP_NEG: GA_PROBE_FIELD_OP(OP_NEG, 0);
    case OP_DBL: GA_PROBE_FIELD_OP(OP_DBL, 0);
    case OP_MUL: GA_PROBE_FIELD_OP(OP_MUL, 0);
    case OP_SQR: GA_PROBE_FIELD_OP(OP_SQR, 0);
    case OP_INV: GA_PROBE_FIELD_OP(OP_INV, 0);
    case OP_FROM_MONT: GA_PROBE_FIELD_OP(OP_FROM_MONT, 0);
    case OP_TO_MONT: GA_PROBE_FIELD_OP(OP_TO_MONT, 0);
    case OP_MUL_SMALL: GA_PROBE_FIELD_OP(OP_MUL_SMALL, 0);
    case OP_F29_FROM_MEM: GA_PROBE_FIELD_OP(OP_F29_FROM_MEM, 0);
    case OP_F29_UNPACK: GA_PROBE_FIELD_OP(OP_F29_UNPACK, 0);
    case OP_F29_HAT_PACKED: GA_PROBE_FIELD_OP(OP_F29_HAT_PACKED, 0);
    case OP_F29_TO_MEM: GA_PROBE_FIELD_OP(OP_F29_TO_MEM, 0);
    case OP_F29_PACK_CANONICAL: GA_PROBE_FIELD_OP(OP_F29_PACK_CANONICAL, 0);
    case OP_F29_PACK_HAT: GA_PROBE_FIELD_OP(OP_F29_PACK_HAT, 0);
    case OP_F29_NORMALIZE: GA_PROBE_FIELD_OP(OP_F29_NORMALIZE, 0);
    case OP_F29_ADD: GA_PROBE_FIELD_OP(OP_F29_ADD, 0);
    case OP_F29_ADD_RAW: GA_PROBE_FIELD_OP(OP_F29_ADD_RAW, 0);
    // the subtraction constants the kernels use (msm_bucket.hip.h, msm_lazy.hip.h, ntt.hip.h, plonk.hip.h, field29.hip.h)
    case OP_F29_SUB:
        if (k == 2) GA_PROBE_FIELD_OP(OP_F29_SUB, 2);
        if (k == 4) GA_PROBE_FIELD_OP(OP_F29_SUB, 4);
        if (k == 8) GA_PROBE_FIELD_OP(OP_F29_SUB, 8);
        return PROBE_BAD_ARGS;
    case OP_F29_SUB_RAW:
        if (k == 4) GA_PROBE_FIELD_OP(OP_F29_SUB_RAW, 4);
        if (k == 8) GA_PROBE_FIELD_OP(OP_F29_SUB_RAW, 8);
        return PROBE_BAD_ARGS;
    case OP_F29_SUB_WIDE:   // <K, W> = <4, 4>
        if (k == 4) GA_PROBE_FIELD_OP(OP_F29_SUB_WIDE, 4);
        return PROBE_BAD_ARGS;
    case OP_F29_MUL: GA_PROBE_FIELD_OP(OP_F29_MUL, 0);
    case OP_F29_SQR: GA_PROBE_FIELD_OP(OP_F29_SQR, 0);
    case OP_F29_MUL_SUB:
        if (k == 8) GA_PROBE_FIELD_OP(OP_F29_MUL_SUB, 8);
        if constexpr (HasFp2<P>::value) {
            if (k == P::FP2Z_K) GA_PROBE_FIELD_OP(OP_F29_MUL_SUB, P::FP2Z_K);
        }
        return PROBE_BAD_ARGS;
    case OP_F29_PARTIAL_REDUCE: GA_PROBE_FIELD_OP(OP_F29_PARTIAL_REDUCE, 0);
    case OP_F29_REDUCE_3P: GA_PROBE_FIELD_OP(OP_F29_REDUCE_3P, 0);
    case OP_F29_IS_ZERO_MOD_P: GA_PROBE_FIELD_OP(OP_F29_IS_ZERO_MOD_P, 0);
    case OP_F29_INV: GA_PROBE_FIELD_OP(OP_F29_INV, 0);
    }
    if constexpr (!HasG1<P>::value) {
        if (op == OP_DIGIT_WALK)
            return k >= 4 && k <= 24 ? launch(probe_digits_kernel<P>, 64, 9, 2 * DIGIT_WINDOWS, k, GA_PROBE_ARGS) : PROBE_BAD_ARGS;
    }
    if constexpr (HasFp2<P>::value) {
        switch (op) {
        case OP_F29X2_MUL: GA_PROBE_FIELD_OP(OP_F29X2_MUL, 0);
        case OP_F29X2_SQR: GA_PROBE_FIELD_OP(OP_F29X2_SQR, 0);
        case OP_F29X2_MUL_SUB:
            if (k == P::FP2Z_K) GA_PROBE_FIELD_OP(OP_F29X2_MUL_SUB, P::FP2Z_K);
            return PROBE_BAD_ARGS;
        case OP_F29X2_INV: GA_PROBE_FIELD_OP(OP_F29X2_INV, 0);
        }
        if (op >= OP_PT2_BASE && op <= OP_PT2_BASE + 4) return run_point<Fe2<P>>(op - OP_PT2_BASE + OP_PT_ADD29, k, GA_PROBE_ARGS);
    }
    if constexpr (HasG1<P>::value) {
        if (op >= OP_PT_ADD29 && op <= OP_PT_MADD29_COMPLETE) return run_point<Fe<P>>(op, k, GA_PROBE_ARGS);
    }
    return PROBE_BAD_ARGS;
}

}  // namespace

// field: 0 BN254 Fp, 1 BN254 Fr, 2 BLS12-381 Fp, 3 BLS12-381 Fr, 4 BLS12-377 Fp (G1 point formulas, no Fp2: the ops 40..43, the
// point ops 60..64 and f29_mul_sub with k = FP2Z_K are refused), 5 BLS12-377 Fr.  in: n elements of in_words words, out: n elements of out_words
// words, both host memory; the word counts must be the op's (a mismatch is refused, nothing is launched).  k: the template constant
// of the subtractions, the factor of mul_small, the number of chained applications of a point formula, the window width of the digits.  Returns 0, 1 (bad
// arguments) or 2 (a HIP call failed).
extern "C" __attribute__((visibility("default"))) int ga_probe_run(int field, int op, int k, const uint32_t* in, size_t n, size_t in_words,
                                                                    uint32_t* out, size_t out_words) {
    switch (field) {
    case 0: return run_field<BN254_Fp>(op, k, GA_PROBE_ARGS);
    case 1: return run_field<BN254_Fr>(op, k, GA_PROBE_ARGS);
    case 2: return run_field<BLS12_381_Fp>(op, k, GA_PROBE_ARGS);
    case 3: return run_field<BLS12_381_Fr>(op, k, GA_PROBE_ARGS);
    case 4: return run_field<BLS12_377_Fp>(op, k, GA_PROBE_ARGS);
    case 5: return run_field<BLS12_377_Fr>(op, k, GA_PROBE_ARGS);
    }
    return PROBE_BAD_ARGS;
}

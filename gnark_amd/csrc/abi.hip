// extern "C" surface of libgnark_amd.so (include/gnark_amd.h): context, buffers, MSM, NTT, group helpers,
// profiling.  The Groth16 entry points are g16_abi.hip, under the same rule (their drivers: groth16.hip, g16_key.hip.h,
// g16_io.hip.h).  Every entry point selects the context's device itself and takes the context mutex (one proof at a time per device,
// as icicle.go:821-823).  An entry point checks its arguments, reads its knobs, takes the lock and makes ONE dispatch into the driver
// of its call family, which lives beside that family's kernels; the runtime under all of them is ctx.hip.
#include <vector>

#include "hostops.hip.h"

namespace ga {

typedef CtxLock Lock;

// ---- the run-time knobs of the point and Fr vector calls (their drivers are declared in common.hip.h) --------------------------
// They are NOT part of Tunables (no other code reads them): the entry point reads them from the environment itself with env_u64 /
// env_int / env_flag, once per call, under the context's lock, before any launch, and hands them to its driver.
//   ga_msm, ga_msm_windows -- and, through the same driver (msm_run), the MSMs of ga_g16_prove over un-pinned vectors (precompute = -1),
//   of ga_g16_commit and of ga_plonk_verify
//     GA_MSM_MAX_CHUNK      points per launch sequence (the one knob of this table that IS in Tunables, msm_max_chunk: the prover reads
//                           it without an entry point of this file; 0 = only the 2^31 pair space of one sequence; tests force a few
//                           hundred so that every vector takes several chunks)
//   ga_batch_scalar_mul (and _plan)
//     GA_FIXED_BASE_C       force the window width (2 .. 20; 0 or anything else = planned, 4 .. 18; tests run several widths at small n)
//     GA_FIXED_BASE_CHUNK   scalars per pass (0 = 2^22, at most 2^30; tests force a small chunk)
//   ga_kzg_to_lagrange_g1, ga_lagrange_coeffs
//     GA_EC_NTT_UNIFORM     0: the lanes of every stage are consecutive butterflies of one group (the A/B of tools/to_lagrange_bench.py);
//                           default 1: from stage 6 on the lanes of a wave share their scalar
//   ga_scale_points
//     GA_SCALE_WINDOW       0: the plain double-and-add ladder (the A/B of tools/scale_points_bench.py); default 1: signed 4-bit windows
//     GA_SCALE_CHUNK        points per pass (0 = 2^20, at most 2^30; tests force a small chunk)
//   ga_check_points; the checked key reads take GA_CHECK_NAIVE as well (check_naive_knob)
//     GA_CHECK_NAIVE        1: the definitional test [r - 1]P = -P on the plain ladder (the A/B of tools/check_points_bench.py); default 0
//     GA_CHECK_CHUNK        points per pass (0 = 2^20, at most 2^30; tests force a small chunk)
//   ga_sparse_point_sums
//     GA_SPARSE_CHUNK       general terms (products) per pass (0 = 2^20, at most 2^30; tests force a small chunk)
//     GA_SPARSE_SEGMENT     terms, or partial sums, per lane of the row sums (0 or 1 = 16; tests force 4)
//     GA_SPARSE_ORDER       0: the products in row order (default); 1: sorted by coefficient id (the A/B of tools/phase2_init_bench.py)
//   ga_pairing_check
//     GA_PAIRING_CHUNK      pairs per pass (0 = 2^18, at most 2^30; tests force a small chunk)
//   ga_g16_pk_read_mem / _fd (and _checked), ga_g16_key_write_fd   (read in g16_abi.hip)
//     GA_KEY_CHUNK          points per staging pass of the key reader and writer (0 = as many as the 32 MiB staging buffers hold, a
//                           larger value is capped there; the buffers keep their size; tests force 1 and 63 .. 65)
//   ga_plonk_verify           the knobs of the calls it is made of: GA_CHECK_NAIVE, GA_CHECK_CHUNK, GA_SPARSE_CHUNK, GA_SPARSE_SEGMENT,
//                             GA_PAIRING_CHUNK (tests force small chunks so that a few proofs take several passes)
//   ga_fr_sparse_matvec
//     GA_FR_SPARSE_SEGMENT  terms, or partial sums, per lane: 2 .. 2^20; unset, 0 or 1 = the default (FR_SPARSE_DEFAULT_SEGMENT); a
//                           larger value is taken as 2^20; tests force 2
//   ga_plonk_build_z_batch, ga_plonk_quotient_pinned_batch, ga_kzg_open_batch
//     GA_PLONK_BATCH_MAX    most proofs per device pass (1 .. 16, default 16 = the limit of the batched table MSM; tests force several passes)
//   the same three, and the single calls that are their one-proof case: ga_plonk_build_z, ga_plonk_quotient_pinned, ga_kzg_open,
//   ga_fr_poly_evaluate
//     GA_PLONK_SCAN_THREADS threads a segmented scan aims at when it chooses its chunk of 8 .. 256 elements (default 2^13; 0 = default;
//                           tests force small values so that sizes of a few hundred elements take every chunk width)
static PlonkBatchKnobs env_plonk_batch_knobs() {
    const uint64_t b = env_u64("GA_PLONK_BATCH_MAX", PLONK_BATCH_LIMIT), t = env_u64("GA_PLONK_SCAN_THREADS", 0);
    return PlonkBatchKnobs{(uint32_t)(b < 1 ? 1 : b > PLONK_BATCH_LIMIT ? PLONK_BATCH_LIMIT : b), t ? t : 8192};
}
static uint32_t env_segment(const char* name) {   // the two segment knobs, capped
    const uint64_t v = env_u64(name, 0);
    return (uint32_t)(v < (1u << 20) ? v : (1u << 20));
}

// ---- argument checks the entry points share: each sets the error under the entry point's name and returns false -------------------
// (the curve and group ids: an entry point that answers n = 0 before it dispatches names its scope S once, asks
// dispatch_check(S, curve, group) first and dispatches under the same S -- a bad id is never answered with GA_OK)
// n elements whose first has index `first`: at most 2^32 of them, and no index above 2^64 - 1
static bool abi_range_ok(size_t n, uint64_t first) {
    if ((uint64_t)n <= (1ull << 32) && (n == 0 || first <= UINT64_MAX - (uint64_t)n + 1)) return true;
    set_error("%s: n = %zu above 2^32, or first + n above 2^64", current_entry(), n);
    return false;
}

// a host-resident PLONK permutation: every entry in [0, 3n) (a device-resident one is checked by the driver, plonk_build_z)
static bool abi_permutation_ok(const int64_t* permutation, uint64_t n3) {
    for (uint64_t i = 0; i < n3; i++)
        if (permutation[i] < 0 || (uint64_t)permutation[i] >= n3) {
            set_error("%s: permutation[%llu] = %lld is outside [0, 3n)", current_entry(), (unsigned long long)i, (long long)permutation[i]);
            return false;
        }
    return true;
}

// the arguments the single and the batched form of a call share: one check, reported under the name of the entry point that was called
static bool abi_kzg_open_ok(const MsmTable* t, const void* polys, size_t n, const void* points, const void* values_out, const void* h_out) {
    if (abi_bad_argument(!t || !polys || !points || !values_out || !h_out || n == 0, "null argument or empty polynomial")) return false;
    if (t->group != GA_G1 || n - 1 > t->n) {
        set_error("%s: the SRS table must be G1 and hold at least len(p) - 1 = %zu points (it has %zu)", current_entry(), n - 1, t->n);
        return false;
    }
    return true;
}
static bool abi_fft_ok(const Domain* d, const void* data, int direction, int decimation) {
    if (d && data && (direction == GA_FFT_FORWARD || direction == GA_FFT_INVERSE) && (decimation == GA_DIF || decimation == GA_DIT)) return true;
    set_error("%s: bad argument", current_entry());
    return false;
}
static bool abi_compute_h_ok(const Domain* d, const void* a, const void* b, const void* c, uint64_t n_constraints, const void* h_out) {
    if (d && a && b && c && h_out && n_constraints <= ntt_domain_size(d)) return true;
    set_error("%s: bad argument (n_constraints must be <= domain cardinality)", current_entry());
    return false;
}

}  // namespace ga

using namespace ga;

extern "C" {

const char* ga_last_error(void) { return get_error(); }
const char* ga_version(void) { return "gnark_amd 0.1 (gfx950; Groth16/PLONK prover kernels: MSM G1/G2, NTT; BN254, BLS12-381)"; }

int ga_device_count(int* count) try {
    GA_ABI_ENTRY();
    GA_HIP_CHECK(hipGetDeviceCount(count));
    return GA_OK;
} GA_ABI_CATCH

int ga_ctx_create(int device, ga_ctx** out) try {
    GA_ABI_ENTRY();
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        set_error("no HIP device available (%s); libgnark_amd has no CPU fallback", e == hipSuccess ? "count=0" : hipGetErrorString(e));
        return GA_ERR_HIP;
    }
    if (device < 0 || device >= count) {
        set_error("device %d out of range (have %d)", device, count);
        return GA_ERR_INVALID;
    }
    GA_HIP_CHECK(hipSetDevice(device));
    {
        hipDeviceProp_t prop;
        GA_HIP_CHECK(hipGetDeviceProperties(&prop, device));
        if (prop.warpSize != 64) {   // (common.hip.h: every kernel is written for 64-lane wavefronts)
            set_error("device %d runs %d-lane wavefronts; libgnark_amd's kernels need 64 (gfx950)", device, prop.warpSize);
            return GA_ERR_INVALID;
        }
    }
    Ctx* c = new Ctx();
    c->device = device;
    hipStream_t* slots[3 + GA_NUM_LANES] = {&c->lane_stream[0], &c->lane_stream[1], &c->lane_stream[2], &c->lane_stream[3],
                                            &c->copy_stream, &c->slot_stream[0], &c->slot_stream[1]};
    // (measured and dropped, profiles/README.md round 3 batch H: creating the partner lanes -- or the witness lanes -- with the highest
    // stream priority changes nothing: 140.3 / 140.9 ms per proof without, 141.1 / 141.9 / 141.0 with)
    for (int k = 0; k < 3 + GA_NUM_LANES; k++) {
        hipError_t se = hipStreamCreateWithFlags(slots[k], hipStreamNonBlocking);
        if (se != hipSuccess) {
            set_error("hipStreamCreate failed: %s", hipGetErrorString(se));
            for (int q = 0; q < k; q++) hipStreamDestroy(*slots[q]);
            delete c;
            return GA_ERR_HIP;
        }
    }
    c->stream = c->lane_stream[0];
    c->tun.read_env();
    *out = reinterpret_cast<ga_ctx*>(c);
    return GA_OK;
} GA_ABI_CATCH

void ga_ctx_destroy(ga_ctx* h) try {
    GA_ABI_ENTRY();
    if (!h) return;
    Ctx* c = reinterpret_cast<Ctx*>(h);
    hipSetDevice(c->device);
    for (int l = 0; l < GA_NUM_LANES; l++) hipStreamSynchronize(c->lane_stream[l]);
    c->scratch_free_all();
    if (c->spare_domain) ntt_domain_delete(c->spare_domain);
    c->spare_domain = nullptr;
    for (void*& q : c->spare_vectors.p) {
        hipFree(q);
        q = nullptr;
    }
    c->spare_vectors.have = false;
    for (auto& s : c->stages) {
        hipEventDestroy(s.a);
        hipEventDestroy(s.b);
    }
    for (int l = 0; l < GA_NUM_LANES; l++) hipStreamDestroy(c->lane_stream[l]);
    for (int l = 0; l < GA_NUM_LANES; l++)
        if (c->host_pin[l]) hipHostFree(c->host_pin[l]);
    hipStreamDestroy(c->copy_stream);
    hipStreamDestroy(c->slot_stream[0]);
    hipStreamDestroy(c->slot_stream[1]);
    delete c;
} GA_ABI_CATCH_VOID

int ga_device_info(ga_ctx* h, char* name, size_t name_len, uint64_t* total_bytes, uint64_t* free_bytes) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    Lock l(c);
    hipDeviceProp_t p;
    GA_HIP_CHECK(hipGetDeviceProperties(&p, c->device));
    if (name && name_len) snprintf(name, name_len, "%s (%s, %d CUs)", p.name, p.gcnArchName, p.multiProcessorCount);
    size_t f = 0, t = 0;
    GA_HIP_CHECK(hipMemGetInfo(&f, &t));
    if (total_bytes) *total_bytes = t;
    if (free_bytes) *free_bytes = f;
    return GA_OK;
} GA_ABI_CATCH

int ga_malloc(ga_ctx* h, size_t bytes, void** dptr) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    Lock l(c);
    hipError_t e = device_malloc(dptr, bytes ? bytes : 16);
    if (e != hipSuccess) {
        set_error("device_malloc(%zu) failed: %s", bytes, device_malloc_error(e));
        return GA_ERR_NOMEM;
    }
    return GA_OK;
} GA_ABI_CATCH

int ga_free(ga_ctx* h, void* dptr) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    Lock l(c);
    GA_HIP_CHECK(hipStreamSynchronize(c->stream));
    GA_HIP_CHECK(hipFree(dptr));
    return GA_OK;
} GA_ABI_CATCH

int ga_copy_to_device(ga_ctx* h, void* dst, const void* src, size_t bytes) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    Lock l(c);
    GA_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    GA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GA_OK;
} GA_ABI_CATCH

int ga_copy_to_host(ga_ctx* h, void* dst, const void* src, size_t bytes) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    Lock l(c);
    GA_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    GA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GA_OK;
} GA_ABI_CATCH

int ga_sync(ga_ctx* h) try {   // (every entry point returns with its own work finished; this waits for both lanes' streams)
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    Lock l(c);
    for (int l = 0; l < GA_NUM_LANES; l++) GA_HIP_CHECK(hipStreamSynchronize(c->lane_stream[l]));
    return GA_OK;
} GA_ABI_CATCH

// ---- MSM (msm.hip.h) ---------------------------------------------------------------------------------------
int ga_msm(ga_ctx* h, int curve, int group, const void* bases, const void* scalars, size_t n, unsigned flags, void* out_jac) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (abi_null_argument(!c || !out_jac || (n && (!bases || !scalars)))) return GA_ERR_INVALID;
    Lock l(c);
    return GA_DISPATCH(Scope::G1_FR, curve, group, return (msm_abi_run<C, G>(c, bases, scalars, n, flags, 0, -1, out_jac, nullptr, nullptr, false)));
} GA_ABI_CATCH

int ga_msm_windows(ga_ctx* h, int curve, int group, const void* bases, const void* scalars, size_t n, unsigned flags, int win_lo,
                   int win_hi, void* out_windows, int* window_bits, int* num_windows) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (abi_null_argument(!c || !out_windows || (n && (!bases || !scalars)))) return GA_ERR_INVALID;
    Lock l(c);
    return GA_DISPATCH(Scope::G1_FR, curve, group,
                       return (msm_abi_run<C, G>(c, bases, scalars, n, flags, win_lo, win_hi, out_windows, window_bits, num_windows, true)));
} GA_ABI_CATCH

// ---- fixed-base batch scalar multiplication (fixed_base.hip.h) ---------------------------------------------
int ga_batch_scalar_mul(ga_ctx* h, int curve, int group, const void* base_affine, const void* scalars, size_t n, unsigned flags,
                        void* out_affine) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    constexpr Scope S = Scope::G1_FR;
    GA_CHECK(dispatch_check(S, curve, group));
    if (n == 0) return GA_OK;
    if (abi_null_argument(!c || !base_affine || !scalars || !out_affine)) return GA_ERR_INVALID;
    if ((flags & GA_RESULT_BITREVERSED) && (n & (n - 1)) != 0) {
        set_error("ga_batch_scalar_mul: GA_RESULT_BITREVERSED needs a power-of-two n (got %zu)", n);
        return GA_ERR_INVALID;
    }
    Lock l(c);
    const int forced_c = env_int("GA_FIXED_BASE_C", 0);
    const uint64_t forced_chunk = env_u64("GA_FIXED_BASE_CHUNK", 0);
    return GA_DISPATCH(S, curve, group, return (fixed_base_run<C, G>(c, base_affine, scalars, n, flags, out_affine, forced_c, forced_chunk)));
} GA_ABI_CATCH

int ga_batch_scalar_mul_plan(int curve, size_t n, int* window_bits, int* num_windows) try {
    GA_ABI_ENTRY();
    if (abi_null_argument(!window_bits || !num_windows)) return GA_ERR_INVALID;
    const int forced_c = env_int("GA_FIXED_BASE_C", 0);
    return GA_DISPATCH(Scope::G1_FR, curve, GA_NO_GROUP, return fixed_base_plan_abi<C>(n, forced_c, window_bits, num_windows));
} GA_ABI_CATCH

// ---- kzg.ToLagrangeG1 (ec_ntt.hip.h) -----------------------------------------------------------------------
int ga_kzg_to_lagrange_g1(ga_ctx* h, int curve, const void* powers_affine, size_t n, unsigned flags, void* out_affine) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    constexpr Scope S = Scope::G1_FR;
    GA_CHECK(dispatch_check(S, curve, GA_NO_GROUP));
    if (n == 0) return GA_OK;
    if (abi_null_argument(!c || !powers_affine || !out_affine)) return GA_ERR_INVALID;
    Lock l(c);
    const int uniform = env_flag("GA_EC_NTT_UNIFORM", 1);
    return GA_DISPATCH(S, curve, GA_NO_GROUP, return (ec_ntt_to_lagrange<C, GA_G1>(c, powers_affine, n, flags, out_affine, uniform)));
} GA_ABI_CATCH

int ga_lagrange_coeffs(ga_ctx* h, int curve, int group, const void* powers_affine, size_t n, unsigned flags, void* out_affine) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    constexpr Scope S = Scope::FULL;
    GA_CHECK(dispatch_check(S, curve, group));
    if (n == 0) return GA_OK;
    if (abi_null_argument(!c || !powers_affine || !out_affine)) return GA_ERR_INVALID;
    Lock l(c);
    const int uniform = env_flag("GA_EC_NTT_UNIFORM", 1);
    return GA_DISPATCH(S, curve, group, return (ec_ntt_to_lagrange<C, G>(c, powers_affine, n, flags, out_affine, uniform)));
} GA_ABI_CATCH

// ---- per-point scalar multiplication (scale_points.hip.h) ---------------------------------------------------
int ga_scale_points(ga_ctx* h, int curve, int group, const void* points_affine, size_t n, int mode, const void* scalars, uint64_t first,
                    unsigned flags, void* out_affine, uint64_t* redone) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    constexpr Scope S = Scope::FULL;
    GA_CHECK(dispatch_check(S, curve, group));
    if (mode != GA_SCALE_EACH && mode != GA_SCALE_ONE && mode != GA_SCALE_POWERS) {
        set_error("ga_scale_points: unknown mode %d", mode);
        return GA_ERR_INVALID;
    }
    if (first != 0 && mode != GA_SCALE_POWERS) {
        set_error("ga_scale_points: first = %llu outside GA_SCALE_POWERS", (unsigned long long)first);
        return GA_ERR_INVALID;
    }
    if ((flags & GA_SCALARS_ON_DEVICE) && mode != GA_SCALE_EACH) {
        set_error("ga_scale_points: GA_SCALARS_ON_DEVICE outside GA_SCALE_EACH (one or two scalars are read on the host)");
        return GA_ERR_INVALID;
    }
    if (!abi_range_ok(n, first)) return GA_ERR_INVALID;
    if (n == 0) {
        if (redone) *redone = 0;
        return GA_OK;
    }
    if (abi_null_argument(!c || !points_affine || !scalars || !out_affine)) return GA_ERR_INVALID;
    Lock l(c);
    const int windowed = env_flag("GA_SCALE_WINDOW", 1);
    const uint64_t forced_chunk = env_u64("GA_SCALE_CHUNK", 0);
    return GA_DISPATCH(S, curve, group,
                       return (scale_points_run<C, G>(c, points_affine, n, mode, scalars, first, flags, out_affine, redone, windowed, forced_chunk)));
} GA_ABI_CATCH

// ---- batch curve and subgroup checks (check_points.hip.h) ---------------------------------------------------
int ga_check_points(ga_ctx* h, int curve, int group, const void* points_affine, size_t n, unsigned flags, uint8_t* status, uint64_t* out4) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    constexpr Scope S = Scope::G1_FR;
    GA_CHECK(dispatch_check(S, curve, group));
    if ((uint64_t)n > (1ull << 32)) {
        set_error("ga_check_points: n = %zu above 2^32", n);
        return GA_ERR_INVALID;
    }
    if (abi_null_argument(!out4 || (n > 0 && (!c || !points_affine)))) return GA_ERR_INVALID;
    if (n == 0) {
        out4[0] = out4[1] = out4[3] = 0;
        out4[2] = UINT64_MAX;
        return GA_OK;
    }
    Lock l(c);
    const int naive = check_naive_knob();
    const uint64_t forced_chunk = env_u64("GA_CHECK_CHUNK", 0);
    return GA_DISPATCH(S, curve, group, return (check_points_run<C, G>(c, points_affine, n, flags, status, out4, naive, forced_chunk)));
} GA_ABI_CATCH

// ---- products of pairings (pairing.hip.h) -----------------------------------------------------------------
int ga_pairing_check(ga_ctx* h, int curve, const void* p_affine, const void* q_affine, size_t n, const uint64_t* group_start, size_t n_groups, unsigned flags,
                     uint8_t* ok, void* gt, uint64_t* out2) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    constexpr Scope S = Scope::FULL;
    GA_CHECK(dispatch_check(S, curve, GA_NO_GROUP));
    if (n_groups == 0) return GA_OK;
    if ((uint64_t)n > (1ull << 32) || (uint64_t)n_groups >= (1ull << 31)) {
        set_error("ga_pairing_check: n = %zu above 2^32 or n_groups = %zu above 2^31 - 1", n, n_groups);
        return GA_ERR_INVALID;
    }
    if (abi_null_argument(!c || !out2 || (n > 0 && (!p_affine || !q_affine)))) return GA_ERR_INVALID;
    if (!group_start && n_groups != 1) {
        set_error("ga_pairing_check: group_start = NULL is one group of all pairs, n_groups = %zu", n_groups);
        return GA_ERR_INVALID;
    }
    if (group_start) {
        if (group_start[0] != 0 || group_start[n_groups] != n) {
            set_error("ga_pairing_check: group_start runs from %llu to %llu, not from 0 to n = %zu", (unsigned long long)group_start[0],
                      (unsigned long long)group_start[n_groups], n);
            return GA_ERR_INVALID;
        }
        for (size_t g = 0; g < n_groups; g++)
            if (group_start[g + 1] < group_start[g]) {
                set_error("ga_pairing_check: group_start decreases at group %zu (%llu after %llu)", g, (unsigned long long)group_start[g + 1],
                          (unsigned long long)group_start[g]);
                return GA_ERR_INVALID;
            }
    }
    Lock l(c);
    const uint64_t forced_chunk = env_u64("GA_PAIRING_CHUNK", 0);
    return GA_DISPATCH(S, curve, GA_NO_GROUP, return (pairing_run<C>(c, p_affine, q_affine, n, group_start, n_groups, flags, ok, gt, out2, forced_chunk)));
} GA_ABI_CATCH

// ---- sparse point sums (sparse_sums.hip.h) ----------------------------------------------------------------
int ga_sparse_point_sums(ga_ctx* h, int curve, int group, const void* points_affine, size_t n_points, const uint64_t* row_start, size_t n_rows,
                         const uint32_t* terms, const void* coeffs, size_t n_coeffs, unsigned flags, void* out_affine, uint64_t* redone) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    constexpr Scope S = Scope::FULL;
    GA_CHECK(dispatch_check(S, curve, group));
    if (n_rows == 0) {
        if (redone) *redone = 0;
        return GA_OK;
    }
    if ((uint64_t)n_rows >= (1ull << 31) || (uint64_t)n_points > (1ull << 32) || (uint64_t)n_coeffs > (1ull << 32)) {
        set_error("ga_sparse_point_sums: n_rows = %zu (at most 2^31 - 1), n_points = %zu or n_coeffs = %zu (at most 2^32) out of range", n_rows, n_points,
                  n_coeffs);
        return GA_ERR_INVALID;
    }
    if ((flags & GA_RESULT_BITREVERSED) && (n_rows & (n_rows - 1)) != 0) {
        set_error("ga_sparse_point_sums: GA_RESULT_BITREVERSED needs a power-of-two n_rows (got %zu)", n_rows);
        return GA_ERR_INVALID;
    }
    if (abi_null_argument(!c || !row_start || !out_affine || (row_start[n_rows] != 0 && (!points_affine || !terms || !coeffs)))) return GA_ERR_INVALID;
    Lock l(c);
    const uint64_t forced_chunk = env_u64("GA_SPARSE_CHUNK", 0);
    const uint32_t segment = env_segment("GA_SPARSE_SEGMENT");
    const int cid_order = env_u64("GA_SPARSE_ORDER", 0) != 0;
    return GA_DISPATCH(S, curve, group,
                       return (sparse_sums_run<C, G>(c, points_affine, n_points, row_start, n_rows, terms, coeffs, n_coeffs, flags, out_affine, redone,
                                                     forced_chunk, segment, cid_order)));
} GA_ABI_CATCH

// ---- the scalar side of groth16.Setup (fr_sparse.hip.h, fr_setup.hip.h) -----------------------------------
int ga_fr_lagrange_at(ga_ctx* h, int curve, uint64_t n, const void* tau, size_t m, unsigned flags, void* out) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    constexpr Scope S = Scope::FULL;
    GA_CHECK(dispatch_check(S, curve, GA_NO_GROUP));
    int adicity = 0;
    GA_CHECK(GA_DISPATCH(S, curve, GA_NO_GROUP, adicity = C::FrP::ADICITY));
    if (n == 0 || (n & (n - 1)) != 0 || n > (1ull << adicity)) {
        set_error("ga_fr_lagrange_at: n = %llu is not a power of two of at most 2^%d", (unsigned long long)n, adicity);
        return GA_ERR_INVALID;
    }
    if ((uint64_t)m > n) {
        set_error("ga_fr_lagrange_at: m = %zu above n = %llu", m, (unsigned long long)n);
        return GA_ERR_INVALID;
    }
    if (m == 0) return GA_OK;
    if (abi_null_argument(!c || !tau || !out)) return GA_ERR_INVALID;
    Lock l(c);
    return GA_DISPATCH(S, curve, GA_NO_GROUP, return fr_lagrange_run<C>(c, ilog2_u64(n), tau, m, flags, out));
} GA_ABI_CATCH

int ga_fr_sparse_matvec(ga_ctx* h, int curve, const void* x, size_t n_cols, const uint64_t* row_start, size_t n_rows, const uint32_t* terms,
                        const void* coeffs, size_t n_coeffs, const uint8_t* row_class, const void* row_scales, size_t n_classes, unsigned flags,
                        void* out) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    constexpr Scope S = Scope::FULL;
    GA_CHECK(dispatch_check(S, curve, GA_NO_GROUP));
    if (n_rows == 0) return GA_OK;
    if ((uint64_t)n_rows >= (1ull << 31) || (uint64_t)n_cols > (1ull << 32) || (uint64_t)n_coeffs > (1ull << 32)) {
        set_error("ga_fr_sparse_matvec: n_rows = %zu (at most 2^31 - 1), n_cols = %zu or n_coeffs = %zu (at most 2^32) out of range", n_rows, n_cols, n_coeffs);
        return GA_ERR_INVALID;
    }
    if ((row_class == nullptr) != (row_scales == nullptr) || (row_class && (n_classes == 0 || n_classes > 256))) {
        set_error("ga_fr_sparse_matvec: row_class and row_scales come together (both null, or 1 .. 256 classes)");
        return GA_ERR_INVALID;
    }
    if (abi_null_argument(!c || !row_start || !out || (row_start[n_rows] != 0 && (!x || !terms || !coeffs)))) return GA_ERR_INVALID;
    Lock l(c);
    const uint32_t segment = env_segment("GA_FR_SPARSE_SEGMENT");
    return GA_DISPATCH(S, curve, GA_NO_GROUP,
                       return fr_sparse_run<C>(c, x, n_cols, row_start, n_rows, terms, coeffs, n_coeffs, row_class, row_scales, n_classes, flags, out, segment));
} GA_ABI_CATCH

int ga_fr_compact_nonzero(ga_ctx* h, int curve, const void* v, size_t n, unsigned flags, void* out, uint8_t* mask, uint64_t* count) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    constexpr Scope S = Scope::FULL;
    GA_CHECK(dispatch_check(S, curve, GA_NO_GROUP));
    if (abi_bad_argument(!count, "null count")) return GA_ERR_INVALID;
    if ((uint64_t)n >= (1ull << 31)) {
        set_error("ga_fr_compact_nonzero: n = %zu, at most 2^31 - 1", n);
        return GA_ERR_INVALID;
    }
    if (n == 0) {
        *count = 0;
        return GA_OK;
    }
    if (abi_null_argument(!c || !v || !out)) return GA_ERR_INVALID;
    Lock l(c);
    return GA_DISPATCH(S, curve, GA_NO_GROUP, return fr_compact_run<C>(c, v, n, flags, out, mask, count));
} GA_ABI_CATCH

int ga_fr_powers(ga_ctx* h, int curve, const void* scalars, uint64_t first, size_t n, unsigned flags, void* out) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    constexpr Scope S = Scope::FULL;
    GA_CHECK(dispatch_check(S, curve, GA_NO_GROUP));
    if (!abi_range_ok(n, first)) return GA_ERR_INVALID;
    if (n == 0) return GA_OK;
    if (abi_null_argument(!c || !scalars || !out)) return GA_ERR_INVALID;
    Lock l(c);
    return GA_DISPATCH(S, curve, GA_NO_GROUP, return fr_powers_run<C>(c, scalars, first, n, flags, out));
} GA_ABI_CATCH

int ga_msm_plan(int curve, int group, size_t n, int* window_bits, int* num_windows) try {
    GA_ABI_ENTRY();
    return GA_DISPATCH(Scope::G1_FR, curve, group, return msm_plan<C>(G, n, window_bits, num_windows));
} GA_ABI_CATCH

int ga_msm_combine_windows(int curve, int group, const void* windows, int num_windows, int window_bits, void* out_jac) try {
    GA_ABI_ENTRY();
    if (abi_bad_argument(!windows || !out_jac || num_windows <= 0 || window_bits <= 0, "bad argument")) return GA_ERR_INVALID;
    return GA_DISPATCH(Scope::G1_FR, curve, group, (host_jac_horner<typename GroupField<C, G>::F>(windows, num_windows, window_bits, out_jac)));
} GA_ABI_CATCH

// ---- precomputed tables (msm.hip.h) ----------------------------------------------------------------------------
int ga_msm_table_create(ga_ctx* h, int curve, int group, const void* bases, size_t n, unsigned flags, ga_msm_table** out) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (abi_bad_argument(!c || !out || !bases || n == 0, "bad argument")) return GA_ERR_INVALID;
    Lock l(c);
    struct Owner {   // (the table object and its device memory are released on every way out but the successful one)
        MsmTable* t;
        ~Owner() {
            if (t) {
                hipFree(t->d_table);
                delete t;
            }
        }
    } own{new MsmTable{c, curve, group, 0, 0, n, nullptr, 0}};
    GA_CHECK(GA_DISPATCH(Scope::G1_FR, curve, group, return (msm_table_create_run<C, G>(own.t, bases, flags))));
    *out = reinterpret_cast<ga_msm_table*>(own.t);
    own.t = nullptr;
    return GA_OK;
} GA_ABI_CATCH

void ga_msm_table_destroy(ga_msm_table* th) try {
    GA_ABI_ENTRY();
    MsmTable* t = reinterpret_cast<MsmTable*>(th);
    if (!t) return;
    Lock l(t->ctx);
    hipStreamSynchronize(t->ctx->stream);
    t->ctx->forget_table(t->d_table);
    hipFree(t->d_table);
    delete t;
} GA_ABI_CATCH_VOID

int ga_msm_table_info(ga_msm_table* th, int* window_bits, int* num_windows, uint64_t* table_bytes) try {
    GA_ABI_ENTRY();
    MsmTable* t = reinterpret_cast<MsmTable*>(th);
    if (!t) return GA_ERR_INVALID;
    if (window_bits) *window_bits = t->c;
    if (num_windows) *num_windows = t->nwin;
    if (table_bytes) *table_bytes = t->bytes;
    return GA_OK;
} GA_ABI_CATCH

// the three argument shapes of the one run driver; a second caller (the PLONK prover commits from several goroutines) runs beside the
// first on lane 1 (LaneLock)
int ga_msm_table_run(ga_msm_table* th, const void* scalars, unsigned flags, void* out_jac) try {
    GA_ABI_ENTRY();
    MsmTable* t = reinterpret_cast<MsmTable*>(th);
    if (abi_null_argument(!t || !scalars || !out_jac)) return GA_ERR_INVALID;
    LaneLock l(t->ctx);
    return GA_DISPATCH(Scope::G1_FR, t->curve, t->group, return (msm_table_run<C, G>(t, &scalars, 1, flags, 0, -1, out_jac)));
} GA_ABI_CATCH

int ga_msm_table_run_batch(ga_msm_table* th, const void* const* scalars, uint32_t k, unsigned flags, void* out_jacs) try {
    GA_ABI_ENTRY();
    MsmTable* t = reinterpret_cast<MsmTable*>(th);
    if (!t || !scalars || !out_jacs || k == 0 || k > 16) {
        set_error("ga_msm_table_run_batch: null argument or batch size %u outside [1, 16]", k);
        return GA_ERR_INVALID;
    }
    for (uint32_t j = 0; j < k; j++)
        if (!scalars[j]) {
            set_error("ga_msm_table_run_batch: scalars[%u] is null", j);
            return GA_ERR_INVALID;
        }
    if ((uint64_t)k * t->nwin * t->n >= (1ull << 31)) {
        set_error("ga_msm_table_run_batch: %u vectors x %d windows x %zu points exceed the 2^31 pair index space; use smaller batches", k,
                  t->nwin, (size_t)t->n);
        return GA_ERR_INVALID;
    }
    LaneLock l(t->ctx);
    return GA_DISPATCH(Scope::G1_FR, t->curve, t->group, return (msm_table_run<C, G>(t, scalars, k, flags, 0, -1, out_jacs)));
} GA_ABI_CATCH

int ga_msm_table_run_windows(ga_msm_table* th, const void* scalars, unsigned flags, int win_lo, int win_hi, void* out_jac) try {
    GA_ABI_ENTRY();
    MsmTable* t = reinterpret_cast<MsmTable*>(th);
    if (abi_null_argument(!t || !scalars || !out_jac)) return GA_ERR_INVALID;
    if (win_lo < 0 || win_hi > t->nwin || win_hi < win_lo) {
        set_error("ga_msm_table_run_windows: window range [%d,%d) outside [0,%d)", win_lo, win_hi, t->nwin);
        return GA_ERR_INVALID;
    }
    LaneLock l(t->ctx);
    return GA_DISPATCH(Scope::G1_FR, t->curve, t->group, return (msm_table_run<C, G>(t, &scalars, 1, flags, win_lo, win_hi, out_jac)));
} GA_ABI_CATCH

int ga_fr_linear_combination(ga_ctx* h, int curve, uint64_t n, int k, const void* const* vecs, const void* scalars, void* out,
                             int on_device) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (abi_null_argument(!c || !vecs || !scalars || (!out && n))) return GA_ERR_INVALID;
    for (int j = 0; j < k; j++)
        if (!vecs[j]) {
            set_error("ga_fr_linear_combination: vector %d is null", j);
            return GA_ERR_INVALID;
        }
    Lock l(c);
    return GA_DISPATCH(Scope::G1_FR, curve, GA_NO_GROUP, return fr_vec_lincomb<C>(c, n, k, vecs, scalars, out, on_device != 0));
} GA_ABI_CATCH

// p(point) for a polynomial in canonical form (iop.Polynomial.Evaluate / evaluateBlinded, prove.go:1186-1215)
int ga_fr_poly_evaluate(ga_ctx* h, int curve, const void* poly, uint64_t n, const void* point, void* value_out, int on_device) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (abi_null_argument(!c || (!poly && n) || !point || !value_out)) return GA_ERR_INVALID;
    constexpr Scope S = Scope::G1_FR;
    GA_CHECK(dispatch_check(S, curve, GA_NO_GROUP));
    Lock l(c);
    if (n == 0) {   // the zero polynomial
        memset(value_out, 0, 32);
        return GA_OK;
    }
    const uint64_t scan_threads = env_plonk_batch_knobs().scan_threads;
    return GA_DISPATCH(S, curve, GA_NO_GROUP, return kzg_domain_divide<C>(c, poly, n, point, value_out, on_device != 0, scan_threads));
} GA_ABI_CATCH

// kzg.Open(p, point, pk): claimed value p(point) and the commitment to (p(X) - p(point)) / (X - point) over the pinned SRS; and the same
// for `count` polynomials of one length over one SRS (plonk_batch.hip.h: kzg_open_run; the single call is count = 1)
int ga_kzg_open(ga_msm_table* th, const void* poly, size_t n, unsigned flags, const void* point, void* claimed_value_out, void* h_out) try {
    GA_ABI_ENTRY();
    MsmTable* t = reinterpret_cast<MsmTable*>(th);
    if (!abi_kzg_open_ok(t, poly, n, point, claimed_value_out, h_out)) return GA_ERR_INVALID;
    Lock l(t->ctx);
    const PlonkBatchKnobs knobs = env_plonk_batch_knobs();
    return GA_DISPATCH(Scope::G1_FR, t->curve, GA_NO_GROUP, return kzg_open_run<C>(t, &poly, n, 1, flags, point, claimed_value_out, h_out, knobs));
} GA_ABI_CATCH

int ga_kzg_open_batch(ga_msm_table* th, const void* const* polys, size_t n, uint32_t count, unsigned flags, const void* points,
                      void* claimed_values_out, void* h_out) try {
    GA_ABI_ENTRY();
    if (count == 0) return GA_OK;
    MsmTable* t = reinterpret_cast<MsmTable*>(th);
    if (!abi_kzg_open_ok(t, polys, n, points, claimed_values_out, h_out)) return GA_ERR_INVALID;
    for (uint32_t j = 0; j < count; j++)
        if (!polys[j]) {
            set_error("ga_kzg_open_batch: polys[%u] is null", j);
            return GA_ERR_INVALID;
        }
    Lock l(t->ctx);
    const PlonkBatchKnobs knobs = env_plonk_batch_knobs();
    return GA_DISPATCH(Scope::G1_FR, t->curve, GA_NO_GROUP, return kzg_open_run<C>(t, polys, n, count, flags, points, claimed_values_out, h_out, knobs));
} GA_ABI_CATCH

// ---- host group helpers (hostops.hip.h) -------------------------------------------------------------------
int ga_jac_add(int curve, int group, const void* a, const void* b, void* out) try {
    GA_ABI_ENTRY();
    return GA_DISPATCH(Scope::G1_FR, curve, group, (host_jac_add<typename GroupField<C, G>::F>(a, b, out)));
} GA_ABI_CATCH

int ga_jac_to_affine(int curve, int group, const void* a, void* out) try {
    GA_ABI_ENTRY();
    return GA_DISPATCH(Scope::G1_FR, curve, group, (host_jac_to_affine<typename GroupField<C, G>::F>(a, out)));
} GA_ABI_CATCH

int ga_jac_scalar_mul(int curve, int group, const void* a, const void* k, void* out) try {
    GA_ABI_ENTRY();
    return GA_DISPATCH(Scope::G1_FR, curve, group, (host_jac_scalar_mul<typename GroupField<C, G>::F>(host_load_jac<typename GroupField<C, G>::F>(a), k, out)));
} GA_ABI_CATCH

// ---- NTT ------------------------------------------------------------------------------------------------
int ga_domain_create(ga_ctx* h, int curve, uint64_t cardinality, ga_domain** out) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (abi_bad_argument(!c || !out || cardinality == 0, "bad argument")) return GA_ERR_INVALID;
    Lock l(c);
    Domain* d = nullptr;
    GA_CHECK(GA_DISPATCH(Scope::G1_FR, curve, GA_NO_GROUP, return ntt_domain_new<C>(c, cardinality, &d)));
    *out = reinterpret_cast<ga_domain*>(d);
    return GA_OK;
} GA_ABI_CATCH

void ga_domain_destroy(ga_domain* dh) try {
    GA_ABI_ENTRY();
    if (!dh) return;
    Domain* d = reinterpret_cast<Domain*>(dh);
    Lock l(ntt_domain_ctx(d));
    hipStreamSynchronize(ntt_domain_ctx(d)->stream);
    ntt_domain_delete(d);
} GA_ABI_CATCH_VOID

// ga_fft_batch: `count` transforms of one size in ONE launch chain: what a loop of fft.Domain.FFT / FFTInverse over vectors of one
// domain does (PLONK's L, R, O and h1..h3, prove.go of backend/plonk; the three chains of computeH,
// backend/groth16/bn254/prove.go:362-368).  data = count vectors of `cardinality` elements, contiguous.  ga_fft is count = 1.
int ga_fft(ga_domain* dh, void* data, int direction, int decimation, int on_coset, int on_device) try {
    GA_ABI_ENTRY();
    Domain* d = reinterpret_cast<Domain*>(dh);
    if (!abi_fft_ok(d, data, direction, decimation)) return GA_ERR_INVALID;
    Lock l(ntt_domain_ctx(d));
    return ntt_domain_fft_run(d, data, 1, direction, decimation, on_coset, on_device != 0);
} GA_ABI_CATCH

int ga_fft_batch(ga_domain* dh, void* data, uint32_t count, int direction, int decimation, int on_coset, int on_device) try {
    GA_ABI_ENTRY();
    if (count == 0) return GA_OK;
    Domain* d = reinterpret_cast<Domain*>(dh);
    if (!abi_fft_ok(d, data, direction, decimation)) return GA_ERR_INVALID;
    Lock l(ntt_domain_ctx(d));
    return ntt_domain_fft_run(d, data, count, direction, decimation, on_coset, on_device != 0);
} GA_ABI_CATCH

static int plonk_args_from(const ga_plonk_quotient_in* in, bool need_fixed, bool need_var, PlonkQuotientArgs* a) {
    memset(a, 0, sizeof(*a));
    if (in->nb_bsb > (uint32_t)PLONK_MAX_BSB) {
        set_error("plonk: more than %d BSB22 gates", PLONK_MAX_BSB);
        return GA_ERR_INVALID;
    }
    a->nb_bsb = in->nb_bsb;
    const void* fixed[PLONK_NB_FIXED] = {in->l, in->r, in->o, in->z, in->ql, in->qr, in->qm, in->qo, in->qk, in->s1, in->s2, in->s3};
    const bool is_fixed[PLONK_NB_FIXED] = {false, false, false, false, true, true, true, true, false, true, true, true};
    for (int k = 0; k < PLONK_NB_FIXED; k++) {
        if ((is_fixed[k] ? need_fixed : need_var) && !fixed[k]) {
            set_error("plonk: polynomial %d of the input is null", k);
            return GA_ERR_INVALID;
        }
        a->polys[k] = fixed[k];
    }
    for (uint32_t k = 0; k < in->nb_bsb; k++) {
        if ((need_fixed && (!in->qcp || !in->qcp[k])) || (need_var && (!in->pi2 || !in->pi2[k]))) {
            set_error("plonk: null Qcp / Pi2 polynomial %u", k);
            return GA_ERR_INVALID;
        }
        a->polys[PLONK_NB_FIXED + 2 * k] = in->qcp ? in->qcp[k] : nullptr;
        a->polys[PLONK_NB_FIXED + 2 * k + 1] = in->pi2 ? in->pi2[k] : nullptr;
    }
    if (need_var && (!in->bl || !in->br || !in->bo || !in->bz || !in->alpha || !in->beta || !in->gamma)) {
        set_error("plonk: blinding polynomials and challenges are required");
        return GA_ERR_INVALID;
    }
    a->lagrange_mask = in->lagrange_mask;
    a->on_device = (in->flags & GA_PLONK_ON_DEVICE) != 0;
    a->bl = in->bl; a->br = in->br; a->bo = in->bo; a->bz = in->bz;
    a->alpha = in->alpha; a->beta = in->beta; a->gamma = in->gamma;
    return GA_OK;
}

int ga_plonk_quotient(ga_domain* dh0, ga_domain* dh1, const ga_plonk_quotient_in* in, void* h_out) try {
    GA_ABI_ENTRY();
    Domain *d0 = reinterpret_cast<Domain*>(dh0), *d1 = reinterpret_cast<Domain*>(dh1);
    if (!d0 || !d1 || !in || !h_out || ntt_domain_curve(d0) != ntt_domain_curve(d1) || ntt_domain_ctx(d0) != ntt_domain_ctx(d1)) {
        set_error("ga_plonk_quotient: null argument, or the two domains differ in curve/context");
        return GA_ERR_INVALID;
    }
    Ctx* c = ntt_domain_ctx(d0);
    Lock l(c);
    PlonkQuotientArgs a;
    GA_CHECK(plonk_args_from(in, true, true, &a));
    return GA_DISPATCH(Scope::G1_FR, ntt_domain_curve(d0), GA_NO_GROUP, return plonk_domain_quotient<C>(d0, d1, a, h_out));
} GA_ABI_CATCH

int ga_plonk_pk_create(ga_domain* dh0, ga_domain* dh1, const ga_plonk_quotient_in* in, ga_plonk_pk** out) try {
    GA_ABI_ENTRY();
    Domain *d0 = reinterpret_cast<Domain*>(dh0), *d1 = reinterpret_cast<Domain*>(dh1);
    if (!d0 || !d1 || !in || !out || ntt_domain_curve(d0) != ntt_domain_curve(d1) || ntt_domain_ctx(d0) != ntt_domain_ctx(d1)) {
        set_error("ga_plonk_pk_create: null argument, or the two domains differ in curve/context");
        return GA_ERR_INVALID;
    }
    Ctx* c = ntt_domain_ctx(d0);
    Lock l(c);
    PlonkQuotientArgs a;
    GA_CHECK(plonk_args_from(in, true, false, &a));
    PlonkFixed* fx = nullptr;
    GA_CHECK(GA_DISPATCH(Scope::G1_FR, ntt_domain_curve(d0), GA_NO_GROUP, return plonk_domain_fixed_create<C>(d0, d1, a, &fx)));
    *out = reinterpret_cast<ga_plonk_pk*>(fx);
    return GA_OK;
} GA_ABI_CATCH

void ga_plonk_pk_destroy(ga_plonk_pk* p) try {
    GA_ABI_ENTRY();
    PlonkFixed* fx = reinterpret_cast<PlonkFixed*>(p);
    if (!fx) return;
    Ctx* c = ntt_domain_ctx(plonk_fixed_domain0(fx));
    Lock l(c);
    hipStreamSynchronize(c->stream);
    plonk_fixed_delete(fx);
} GA_ABI_CATCH_VOID

int ga_plonk_quotient_pinned(ga_plonk_pk* p, const ga_plonk_quotient_in* in, void* h_out) try {
    GA_ABI_ENTRY();
    PlonkFixed* fx = reinterpret_cast<PlonkFixed*>(p);
    if (abi_null_argument(!fx || !in || !h_out)) return GA_ERR_INVALID;
    Domain* d0 = plonk_fixed_domain0(fx);
    Ctx* c = ntt_domain_ctx(d0);
    Lock l(c);
    PlonkQuotientArgs a;
    GA_CHECK(plonk_args_from(in, false, true, &a));
    const uint64_t scan_threads = env_plonk_batch_knobs().scan_threads;
    return GA_DISPATCH(Scope::G1_FR, ntt_domain_curve(d0), GA_NO_GROUP, return plonk_domain_quotient_pinned<C>(fx, a, scan_threads, h_out));
} GA_ABI_CATCH

int ga_plonk_build_z(ga_domain* dh0, const void* lv, const void* rv, const void* ov, const int64_t* permutation, const void* beta,
                     const void* gamma, int on_device, void* z_out) try {
    GA_ABI_ENTRY();
    Domain* d0 = reinterpret_cast<Domain*>(dh0);
    if (abi_null_argument(!d0 || !lv || !rv || !ov || !permutation || !beta || !gamma || !z_out)) return GA_ERR_INVALID;
    Ctx* c = ntt_domain_ctx(d0);
    Lock l(c);
    if (!on_device && !abi_permutation_ok(permutation, 3 * ntt_domain_size(d0))) return GA_ERR_INVALID;
    const uint64_t scan_threads = env_plonk_batch_knobs().scan_threads;
    return GA_DISPATCH(Scope::G1_FR, ntt_domain_curve(d0), GA_NO_GROUP,
                       return plonk_domain_build_z<C>(d0, lv, rv, ov, permutation, beta, gamma, scan_threads, on_device != 0, z_out));
} GA_ABI_CATCH

int ga_plonk_build_z_batch(ga_domain* dh0, const void* lv, const void* rv, const void* ov, const int64_t* permutation, const void* betas,
                           const void* gammas, uint32_t count, int on_device, void* z_out) try {
    GA_ABI_ENTRY();
    if (count == 0) return GA_OK;
    Domain* d0 = reinterpret_cast<Domain*>(dh0);
    if (abi_null_argument(!d0 || !lv || !rv || !ov || !permutation || !betas || !gammas || !z_out)) return GA_ERR_INVALID;
    Ctx* c = ntt_domain_ctx(d0);
    Lock l(c);
    if (!on_device && !abi_permutation_ok(permutation, 3 * ntt_domain_size(d0))) return GA_ERR_INVALID;
    const PlonkBatchKnobs knobs = env_plonk_batch_knobs();
    return GA_DISPATCH(Scope::G1_FR, ntt_domain_curve(d0), GA_NO_GROUP,
                       return plonk_domain_build_z_batch<C>(d0, lv, rv, ov, permutation, betas, gammas, count, knobs, on_device != 0, z_out));
} GA_ABI_CATCH

int ga_plonk_quotient_pinned_batch(ga_plonk_pk* p, const ga_plonk_quotient_in* ins, uint32_t count, void* h_out) try {
    GA_ABI_ENTRY();
    if (count == 0) return GA_OK;
    PlonkFixed* fx = reinterpret_cast<PlonkFixed*>(p);
    if (abi_null_argument(!fx || !ins || !h_out)) return GA_ERR_INVALID;
    Domain* d0 = plonk_fixed_domain0(fx);
    Ctx* c = ntt_domain_ctx(d0);
    Lock l(c);
    std::vector<PlonkQuotientArgs> a(count);
    for (uint32_t j = 0; j < count; j++) {
        if (ins[j].nb_bsb != ins[0].nb_bsb || ins[j].lagrange_mask != ins[0].lagrange_mask || ins[j].flags != ins[0].flags) {
            set_error("ga_plonk_quotient_pinned_batch: ins[%u] differs from ins[0] in nb_bsb, lagrange_mask or flags", j);
            return GA_ERR_INVALID;
        }
        GA_CHECK(plonk_args_from(&ins[j], false, true, &a[j]));
    }
    const PlonkBatchKnobs knobs = env_plonk_batch_knobs();
    return GA_DISPATCH(Scope::G1_FR, ntt_domain_curve(d0), GA_NO_GROUP, return plonk_domain_quotient_pinned_batch<C>(fx, a.data(), count, knobs, h_out));
} GA_ABI_CATCH

// ---- plonk.Verify for many proofs under one key (plonk_verify.hip.h) ---------------------------------------------------------------
// No curve argument: the curve is the domain's.  The key is Scope::FULL (the verifier ends in a pairing).
int ga_plonk_vk_create(ga_domain* dh0, const ga_plonk_vk_in* in, ga_plonk_vk** out) try {
    GA_ABI_ENTRY();
    Domain* d0 = reinterpret_cast<Domain*>(dh0);
    if (abi_null_argument(!d0 || !in || !out)) return GA_ERR_INVALID;
    constexpr Scope S = Scope::FULL;
    GA_CHECK(dispatch_check(S, ntt_domain_curve(d0), GA_NO_GROUP));
    Ctx* c = ntt_domain_ctx(d0);
    Lock l(c);
    PlonkVk* vk = nullptr;
    GA_CHECK(GA_DISPATCH(S, ntt_domain_curve(d0), GA_NO_GROUP, return plonk_vk_new<C>(d0, in, &vk)));
    *out = reinterpret_cast<ga_plonk_vk*>(vk);
    return GA_OK;
} GA_ABI_CATCH

void ga_plonk_vk_destroy(ga_plonk_vk* p) try {
    GA_ABI_ENTRY();
    PlonkVk* vk = reinterpret_cast<PlonkVk*>(p);
    if (!vk) return;
    Ctx* c = ntt_domain_ctx(plonk_vk_domain0(vk));
    Lock l(c);
    hipStreamSynchronize(c->stream);
    plonk_vk_delete(vk);
} GA_ABI_CATCH_VOID

int ga_plonk_verify_scalars(ga_plonk_vk* p, const ga_plonk_proofs* proofs, uint32_t count, unsigned flags, void* rows_out, uint8_t* relation_ok) try {
    GA_ABI_ENTRY();
    if (count == 0) return GA_OK;
    PlonkVk* vk = reinterpret_cast<PlonkVk*>(p);
    if (abi_null_argument(!vk || !proofs || !rows_out || !relation_ok)) return GA_ERR_INVALID;
    if (count > PLONK_VERIFY_MAX_COUNT) {
        set_error("ga_plonk_verify_scalars: count = %u above 2^20", count);
        return GA_ERR_INVALID;
    }
    Domain* d0 = plonk_vk_domain0(vk);
    Ctx* c = ntt_domain_ctx(d0);
    Lock l(c);
    return GA_DISPATCH(Scope::FULL, ntt_domain_curve(d0), GA_NO_GROUP,
                       return plonk_verify_scalars_run<C>(vk, proofs, count, (flags & GA_PLONK_ON_DEVICE) != 0, rows_out, relation_ok));
} GA_ABI_CATCH

int ga_plonk_verify(ga_plonk_vk* p, const ga_plonk_proofs* proofs, uint32_t count, unsigned flags, const void* weights, uint8_t* ok, uint8_t* relation_ok,
                    uint64_t* out2) try {
    GA_ABI_ENTRY();
    if (count == 0) return GA_OK;
    PlonkVk* vk = reinterpret_cast<PlonkVk*>(p);
    if (!vk || !proofs || !ok || !out2) {
        set_error("ga_plonk_verify: null argument%s", out2 ? "" : " (out2)");
        return GA_ERR_INVALID;
    }
    if (abi_bad_argument((flags & GA_PLONK_VERIFY_COMBINED) && !weights, "GA_PLONK_VERIFY_COMBINED without weights")) return GA_ERR_INVALID;
    if (count > PLONK_VERIFY_MAX_COUNT) {
        set_error("ga_plonk_verify: count = %u above 2^20", count);
        return GA_ERR_INVALID;
    }
    Domain* d0 = plonk_vk_domain0(vk);
    Ctx* c = ntt_domain_ctx(d0);
    Lock l(c);
    const PlonkVerifyKnobs knobs{check_naive_knob(), env_u64("GA_CHECK_CHUNK", 0), env_u64("GA_SPARSE_CHUNK", 0), env_u64("GA_PAIRING_CHUNK", 0),
                                 env_segment("GA_SPARSE_SEGMENT")};
    return GA_DISPATCH(Scope::FULL, ntt_domain_curve(d0), GA_NO_GROUP, return plonk_verify_run<C>(vk, proofs, count, flags, weights, ok, relation_ok, out2, knobs));
} GA_ABI_CATCH

int ga_fr_batch_invert(ga_ctx* h, int curve, void* v, uint64_t n, int on_device) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (abi_null_argument(!c || (!v && n))) return GA_ERR_INVALID;
    Lock l(c);
    return GA_DISPATCH(Scope::G1_FR, curve, GA_NO_GROUP, return fr_vec_batch_inverse<C>(c, v, n, on_device != 0));
} GA_ABI_CATCH

// ga_compute_h_batch: computeH for `count` solutions of one circuit (a loop of prove.go:346-389 over the solutions).  a, b, c =
// [count][n_constraints] contiguous; h_out = [count][cardinality], bit-reversed.  ga_compute_h is count = 1.
int ga_compute_h(ga_domain* dh, const void* a, const void* b, const void* cc, uint64_t n_constraints, void* h_out, int on_device) try {
    GA_ABI_ENTRY();
    Domain* d = reinterpret_cast<Domain*>(dh);
    if (!abi_compute_h_ok(d, a, b, cc, n_constraints, h_out)) return GA_ERR_INVALID;
    Lock l(ntt_domain_ctx(d));
    return ntt_domain_compute_h_run(d, a, b, cc, 1, n_constraints, h_out, on_device != 0);
} GA_ABI_CATCH

int ga_compute_h_batch(ga_domain* dh, const void* a, const void* b, const void* cc, uint32_t count, uint64_t n_constraints, void* h_out,
                       int on_device) try {
    GA_ABI_ENTRY();
    if (count == 0) return GA_OK;
    Domain* d = reinterpret_cast<Domain*>(dh);
    if (!abi_compute_h_ok(d, a, b, cc, n_constraints, h_out)) return GA_ERR_INVALID;
    Lock l(ntt_domain_ctx(d));
    return ntt_domain_compute_h_run(d, a, b, cc, count, n_constraints, h_out, on_device != 0);
} GA_ABI_CATCH

// ---- profiling ------------------------------------------------------------------------------------------
int ga_profile_enable(ga_ctx* h, int on) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    Lock l(c);
    c->profiling = on != 0;
    return GA_OK;
} GA_ABI_CATCH

int ga_profile_reset(ga_ctx* h) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    Lock l(c);
    hipStreamSynchronize(c->stream);
    for (auto& s : c->stages) {
        hipEventDestroy(s.a);
        hipEventDestroy(s.b);
    }
    c->stages.clear();
    return GA_OK;
} GA_ABI_CATCH

int ga_profile_read(ga_ctx* h, char* buf, size_t cap) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    Lock l(c);
    GA_HIP_CHECK(hipStreamSynchronize(c->stream));
    std::string out;
    for (auto& s : c->stages) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, s.a, s.b) != hipSuccess) ms = -1;
        char tmp[160];
        snprintf(tmp, sizeof(tmp), "%s=%.6f;", s.name.c_str(), ms);
        out += tmp;
    }
    if (!buf || cap == 0) return GA_ERR_INVALID;
    snprintf(buf, cap, "%s", out.c_str());
    return GA_OK;
} GA_ABI_CATCH

// ---- test / bench support -------------------------------------------------------------------------------
int ga_gen_bases(ga_ctx* h, int curve, int group, uint64_t seed, size_t n, void* bases_dev, void* dlogs_dev) try {   // first = 0 of the next
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    Lock l(c);
    GA_CHECK(GA_DISPATCH(Scope::G1_FR, curve, group, return util_gen_bases<C, G>(c, seed, n, bases_dev, dlogs_dev, 0)));
    GA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GA_OK;
} GA_ABI_CATCH

int ga_gen_bases_at(ga_ctx* h, int curve, int group, uint64_t seed, uint64_t first, size_t n, void* bases_dev, void* dlogs_dev) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    Lock l(c);
    GA_CHECK(GA_DISPATCH(Scope::G1_FR, curve, group, return util_gen_bases<C, G>(c, seed, n, bases_dev, dlogs_dev, first)));
    GA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GA_OK;
} GA_ABI_CATCH

int ga_gen_scalars(ga_ctx* h, int curve, uint64_t seed, size_t n, void* scalars_dev) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    Lock l(c);
    GA_CHECK(GA_DISPATCH(Scope::G1_FR, curve, GA_NO_GROUP, return util_gen_scalars<C>(c, seed, n, scalars_dev)));
    GA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GA_OK;
} GA_ABI_CATCH

int ga_fr_dot(ga_ctx* h, int curve, const void* a_dev, const void* b_dev, size_t n, void* out_host) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    Lock l(c);
    return GA_DISPATCH(Scope::G1_FR, curve, GA_NO_GROUP, return util_fr_dot<C>(c, a_dev, b_dev, n, out_host));
} GA_ABI_CATCH

int ga_fr_vec_mul(ga_ctx* h, int curve, const void* a, const void* b, size_t n, void* out, int on_device) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (abi_null_argument(!c || (n && (!a || !b || !out)))) return GA_ERR_INVALID;
    constexpr Scope S = Scope::G1_FR;
    GA_CHECK(dispatch_check(S, curve, GA_NO_GROUP));
    Lock l(c);
    if (n == 0) return GA_OK;
    return GA_DISPATCH(S, curve, GA_NO_GROUP, return util_fr_vec_mul_run<C>(c, a, b, n, out, on_device != 0));
} GA_ABI_CATCH

int ga_generator_mul(int curve, int group, const void* k, void* out_jac) try {
    GA_ABI_ENTRY();
    return GA_DISPATCH(Scope::G1_FR, curve, group, (host_jac_scalar_mul<typename GroupField<C, G>::F>(to_xyzz(Generator<C, G>::get()), k, out_jac)));
} GA_ABI_CATCH

int ga_clock_probe(ga_ctx* h, uint32_t micros, double* mhz_out) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (abi_bad_argument(!c || !mhz_out || micros == 0, "bad argument")) return GA_ERR_INVALID;
    return util_clock_probe(c, micros, mhz_out);   // (no context lock: it is meant to run BESIDE whatever holds it)
} GA_ABI_CATCH

int ga_microbench(ga_ctx* h, char* buf, size_t cap) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    Lock l(c);
    return util_microbench(c, buf, cap);
} GA_ABI_CATCH

}  // extern "C"

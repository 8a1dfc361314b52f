// extern "C" surface of libgnark_amd.so (include/gnark_amd.h): context, buffers, MSM, NTT, group helpers,
// profiling.  Groth16 lives in groth16.hip (the prover and its entry points; keys in g16_key.hip.h, key files and proof bytes in
// g16_io.hip.h).  Every entry point selects the context's device itself and takes the context mutex (one proof at a time per device,
// as icicle.go:821-823).
#include <stdarg.h>
#include <stdlib.h>

#include <memory>
#include <new>
#include <vector>

#include "hostops.hip.h"

namespace ga {

static thread_local char g_err[1024] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char* get_error() { return g_err; }

int abi_exception_code(const char* entry) noexcept {
    try {
        throw;   // (Lippincott function: re-raise the exception being handled to classify it)
    } catch (const std::bad_alloc&) {
        set_error("out of host memory (std::bad_alloc) under %s", entry);
        return GA_ERR_NOMEM;
    } catch (const std::exception& e) {
        set_error("internal error under %s: %s", entry, e.what());
        return GA_ERR_STATE;
    } catch (...) {
        set_error("internal error under %s: unknown exception", entry);
        return GA_ERR_STATE;
    }
}
static thread_local const char* g_entry = "";
EntryScope::EntryScope(const char* name) : prev(g_entry) { g_entry = name; }
EntryScope::~EntryScope() { g_entry = prev; }
const char* current_entry() { return g_entry; }

// ---- which (curve, group) pairs are built, and the answer for one that is not (common.hip.h: dispatch) ----------------------------
// what the two functions below need of a curve id at run time, read from the tags of GA_CURVES; name == nullptr: no such curve
struct CurveInfo {
    const char* name;
    bool has_g2;
    const char* no_g2;
};
template <class C>
static constexpr const char* no_g2_reason() {
    if constexpr (C::HAS_G2) return "";
    else return C::NO_G2;
}
static CurveInfo curve_info(int curve) {
#define GA_CURVE_INFO(T) \
    if (curve == T::ID) return CurveInfo{T::NAME, T::HAS_G2, no_g2_reason<T>()};
    GA_CURVES(GA_CURVE_INFO)
#undef GA_CURVE_INFO
    return CurveInfo{nullptr, false, ""};
}
static bool group_exists(GroupArg group) { return !group.given || group.id == GA_G1 || group.id == GA_G2; }
bool dispatch_built(Scope scope, int curve, GroupArg group) {
    const CurveInfo ci = curve_info(curve);
    return ci.name && (scope == Scope::G1_FR || ci.has_g2) && group_exists(group) && (group.id != GA_G2 || ci.has_g2);
}
int dispatch_refuse(Scope scope, int curve, GroupArg group) {
    const CurveInfo ci = curve_info(curve);
    const char* entry = current_entry();
    if (!ci.name)   // (asked first: with both ids unknown the curve is reported)
        set_error("%s: unknown curve id %d", entry, curve);
    else if (scope == Scope::FULL && !ci.has_g2)
        set_error("%s is not built for %s (curve id %d): that curve has the G1 and Fr calls only, %s", entry, ci.name, curve, ci.no_g2);
    else if (!group_exists(group))
        set_error("%s: unknown group id %d", entry, group.id);
    else   // G2 of a curve without it
        set_error("%s: G2 is not built for %s (curve id %d): that curve has the G1 and Fr calls only, %s", entry, ci.name, curve, ci.no_g2);
    return GA_ERR_INVALID;
}
static uint64_t fnv1a(const char* s) {
    uint64_t h = 1469598103934665603ull;
    for (; *s; s++) h = (h ^ (uint8_t)*s) * 1099511628211ull;
    return h ? h : 1;
}

static std::atomic<int> g_table_c{0};
int table_c_override() { return g_table_c.load(); }
static thread_local int g_lane = 0;
int current_lane() { return g_lane; }
LaneScope::LaneScope(int lane) : prev(g_lane) { g_lane = lane; }
LaneScope::~LaneScope() { g_lane = prev; }

static thread_local char g_alloc_why[160] = {0};
const char* device_malloc_error(hipError_t e) { return g_alloc_why[0] ? g_alloc_why : hipGetErrorString(e); }

hipError_t device_malloc_bytes(void** p, size_t bytes) {
    // The last GA_HBM_RESERVE_MB (default 1024) MiB of the device stay free for the runtime's own dispatch-time allocations.
    // The reserve is a rule about what THIS allocation leaves behind, so it is checked before the hipMalloc, under the device's
    // mutex (two lanes cannot both pass on the same free bytes).  Allocations below 16 MiB may use the upper half of the reserve: a
    // few-KB buffer is not refused because another process or rank sharing the device has eaten a little into it.
    static const size_t reserve = []() {
        const char* e = getenv("GA_HBM_RESERVE_MB");
        return (size_t)(e ? strtoull(e, nullptr, 10) : 1024ull) << 20;
    }();
    static const size_t small = 16ull << 20;
    // one mutex per DEVICE (the reserve is a per-device rule; ga_g16_prove_multi allocates on several devices from one process and
    // must not serialise them on each other)
    constexpr int MAX_DEV = 64;
    static std::mutex alloc_mu[MAX_DEV];
    *p = nullptr;
    g_alloc_why[0] = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
    std::lock_guard<std::mutex> g(alloc_mu[dev % MAX_DEV]);
    if (reserve) {
        size_t free_b = 0, total_b = 0;
        const size_t floor_b = bytes >= small ? reserve : reserve / 2;
        const hipError_t qe = hipMemGetInfo(&free_b, &total_b);
        if (qe != hipSuccess) {   // without the free-memory figure the reserve cannot be honoured: refuse rather than skip it silently
            (void)hipGetLastError();
            snprintf(g_alloc_why, sizeof(g_alloc_why), "refused: hipMemGetInfo failed (%s), the GA_HBM_RESERVE_MB rule cannot be checked", hipGetErrorString(qe));
            return hipErrorOutOfMemory;
        }
        if (free_b < bytes || free_b - bytes < floor_b) {
            snprintf(g_alloc_why, sizeof(g_alloc_why), "refused: %zu MiB free, the allocation would leave less than the %zu MiB reserve (GA_HBM_RESERVE_MB)",
                     free_b >> 20, reserve >> 20);
            return hipErrorOutOfMemory;
        }
    }
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();   // clear the sticky error: the caller reports this failure itself
        *p = nullptr;
        return e;
    }
    return hipSuccess;
}

int Ctx::scratch_get(const char* base_key, size_t bytes, void** out) {
    // every lane has its own namespace: a lane-1 proof never shares a buffer with the lane-0 work running beside it
    // GA_FAULT_THROW=<entry point> (tests of the ABI's exception barrier): a host allocation failing deep inside that entry point
    if (const uint64_t f = tun.fault_throw.load(std::memory_order_relaxed))
        if (f == fnv1a(current_entry())) throw std::bad_alloc();
    const int lane = current_lane();
    if (lane >= 2 && tun.fault_lane2_nomem.load(std::memory_order_relaxed)) {
        set_error("device scratch '%s@%d': GA_FAULT_LANE2_NOMEM is set (test knob: lanes 2/3 cannot allocate)", base_key, lane);
        return GA_ERR_NOMEM;
    }
    const std::string lane_key = lane ? std::string(base_key) + "@" + std::to_string(lane) : std::string(base_key);
    const char* key = lane_key.c_str();
    std::lock_guard<std::mutex> g(scratch_mu);
    auto it = scratch.find(key);
    if (it != scratch.end() && it->second.bytes >= bytes) {
        *out = it->second.p;
        return GA_OK;
    }
    if (it != scratch.end()) {
        hipFree(it->second.p);
        scratch.erase(it);
    }
    void* p = nullptr;
    // growth slack so that slowly growing requests do not reallocate every time -- capped: 1/8 of a multi-GiB sort buffer is a
    // gigabyte nobody uses (10 GiB of a 2^26 proof's 94 GiB of scratch)
    const size_t slack = bytes / 8 < (64u << 20) ? bytes / 8 : (size_t)(64u << 20);
    size_t want = bytes + slack + 256;
    hipError_t e = device_malloc(&p, want);
    if (e != hipSuccess) {
        set_error("device scratch '%s': device_malloc(%zu) failed: %s", key, want, device_malloc_error(e));
        return GA_ERR_NOMEM;
    }
    scratch[key] = ScratchBuf{p, want, lane};
    *out = p;
    return GA_OK;
}

void Ctx::scratch_free_all() {
    std::lock_guard<std::mutex> g(scratch_mu);
    for (auto& kv : scratch) hipFree(kv.second.p);
    scratch.clear();
}

void Ctx::scratch_free_lanes(int first_lane) {
    std::lock_guard<std::mutex> g(scratch_mu);
    for (auto it = scratch.begin(); it != scratch.end();) {
        if (it->second.lane >= first_lane) {
            hipFree(it->second.p);
            it = scratch.erase(it);
        } else
            ++it;
    }
}

// a 64-bit knob (strtoull), an int knob (atoi), a 0 / 1 knob (anything atoi reads as non-zero is 1); the default when the variable is not set
static uint64_t env_u64(const char* name, uint64_t dflt) {
    const char* e = getenv(name);
    return e ? strtoull(e, nullptr, 10) : dflt;
}
static int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
static int env_flag(const char* name, int dflt) { return env_int(name, dflt) != 0; }
int check_naive_knob() { return env_flag("GA_CHECK_NAIVE", 0); }

void Tunables::read_env() {
    // a prover on another lane may be reading the knobs while lane 0 refreshes them: every field is an atomic, parsed into a
    // local first and stored only when the environment changed it, so a reader never sees the defaults flicker
    auto put64 = [](std::atomic<uint64_t>& f, uint64_t v) {
        if (f.load(std::memory_order_relaxed) != v) f.store(v, std::memory_order_relaxed);
    };
    auto put = [](std::atomic<int>& f, int v) {
        if (f.load(std::memory_order_relaxed) != v) f.store(v, std::memory_order_relaxed);
    };
    put64(msm_max_chunk, env_u64("GA_MSM_MAX_CHUNK", 0));
    put64(reduce_lazy_min, env_u64("GA_REDUCE_LAZY_MIN", 1u << 14));
    put(g16_share_min_pct, (int)env_u64("GA_G16_SHARE_MIN_PCT", 90));
    put(g16_lanes, (int)env_u64("GA_G16_LANES", 2));
    put64(g16_table_budget_pct, env_u64("GA_G16_TABLE_BUDGET_PCT", 0));
    put(g16_split, (int)env_u64("GA_G16_SPLIT", 1));
    put(g16_batch_tables, (int)env_u64("GA_G16_BATCH_TABLES", 1));
    {
        const uint64_t b = env_u64("GA_G16_BATCH_MAX", 16);
        put(g16_batch_max, (int)(b < 1 ? 1 : b > 16 ? 16 : b));
    }
    put(ntt_wave_local, (int)env_u64("GA_NTT_WAVE_LOCAL", 1));
    put(ntt_direct, (int)env_u64("GA_NTT_DIRECT", 1));
    put(table_c, (int)env_u64("GA_TABLE_C", 0));
    put(msm_exact_redo, (int)env_u64("GA_MSM_EXACT_REDO", 0));
    put64(msm_fuse_min, env_u64("GA_MSM_FUSE_MIN", 1ull << 21));
    put64(msm_task_exact_min, env_u64("GA_MSM_TASK_EXACT_MIN", 1ull << 25));
    put(msm_xcd, (int)env_u64("GA_MSM_XCD", 3));
    {
        const uint64_t g = env_u64("GA_MSM_P1_GRID", 512);
        put64(msm_p1_grid, g ? g : 1);
    }
    {
        const char* e = getenv("GA_FAULT_THROW");
        put64(fault_throw, (e && *e) ? fnv1a(e) : 0);
    }
    put(fault_lane2_nomem, (int)env_u64("GA_FAULT_LANE2_NOMEM", 0));
    const int grp = (int)env_u64("GA_MSM_GROUP", 0);
    put(msm_group, (grp >= 2 && grp <= 256 && (grp & (grp - 1)) == 0) ? grp : 0);
    const uint64_t seg = env_u64("GA_MSM_MIN_SEG", 256);
    if (seg >= 32) put64(msm_min_seg, seg);
    g_table_c = table_c.load();
}

typedef CtxLock Lock;

// ---- the run-time knobs of the point and Fr vector calls (their drivers are declared in common.hip.h) --------------------------
// They are NOT part of Tunables (no other code reads them): the entry point reads them from the environment itself with env_u64 /
// env_int / env_flag, once per call, under the context's lock, before any launch, and hands them to its driver.
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

// Bring inputs to the device when they are host pointers.
struct Staged {
    Ctx* ctx;
    const void* dev = nullptr;
    void* owned = nullptr;
    int stage(const void* p, size_t bytes, bool on_device) {
        if (on_device || bytes == 0) {
            dev = p;
            return GA_OK;
        }
        hipError_t e = device_malloc(&owned, bytes);
        if (e != hipSuccess) {
            set_error("device_malloc(%zu) failed: %s", bytes, device_malloc_error(e));
            return GA_ERR_NOMEM;
        }
        GA_HIP_CHECK(hipMemcpyAsync(owned, p, bytes, hipMemcpyHostToDevice, ctx->work_stream()));
        GA_HIP_CHECK(hipStreamSynchronize(ctx->work_stream()));   // host memory must not be referenced after return
        dev = owned;
        return GA_OK;
    }
    ~Staged() {
        if (owned) hipFree(owned);
    }
};

template <class C, int G>
static int msm_impl(Ctx* ctx, const void* bases, const void* scalars, size_t n, unsigned flags, int win_lo, int win_hi,
                    void* out, int* c_out, int* nwin_out, bool want_windows) {
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
    // Split along the point axis when one call would overflow the 2^31 (point, window) pair space -- the analogue of
    // msmChunkedG1/G2 (icicle.go:362-467); partial results are added on the host.  Never needed up to 2^26 points.
    size_t max_chunk = ((size_t)1 << 31) / (size_t)(win_hi - win_lo) - 1;
    if (ctx->tun.msm_max_chunk > 0 && ctx->tun.msm_max_chunk < max_chunk)   // GA_MSM_MAX_CHUNK, like ICICLE's chunk-cap override (icicle.go:577-584)
        max_chunk = (size_t)ctx->tun.msm_max_chunk;
    if (!want_windows && n <= max_chunk) {   // the usual case: one launch sequence, the Horner step shares the window reduction's host chain
        Staged sb{ctx}, ss{ctx};
        GA_CHECK(sb.stage(bases, n * sizeof(Affine<F>), flags & GA_BASES_ON_DEVICE));
        GA_CHECK(ss.stage(scalars, n * 32, flags & GA_SCALARS_ON_DEVICE));
        XYZZ<F> sum;
        GA_CHECK((msm_windows_device<C, G>(ctx, sb.dev, ss.dev, n, (flags & GA_SCALARS_MONTGOMERY) != 0, c, win_lo, win_hi, &sum, true)));
        for (int k = 0; k < c * win_lo; k++) sum = dbl(sum);
        host_store_jac<F>(out, sum);
        return GA_OK;
    }
    std::vector<XYZZ<F>> W(win_hi - win_lo, xyzz_inf<F>());
    for (size_t done = 0; done < n || n == 0; ) {
        const size_t cn = n - done < max_chunk ? n - done : max_chunk;
        Staged sb{ctx}, ss{ctx};
        const char* bp = reinterpret_cast<const char*>(bases) + done * sizeof(Affine<F>);
        const char* sp = reinterpret_cast<const char*>(scalars) + done * 32;
        GA_CHECK(sb.stage(bp, cn * sizeof(Affine<F>), flags & GA_BASES_ON_DEVICE));
        GA_CHECK(ss.stage(sp, cn * 32, flags & GA_SCALARS_ON_DEVICE));
        std::vector<XYZZ<F>> part(win_hi - win_lo);
        GA_CHECK((msm_windows_device<C, G>(ctx, sb.dev, ss.dev, cn, (flags & GA_SCALARS_MONTGOMERY) != 0, c, win_lo, win_hi, part.data())));
        for (size_t w = 0; w < W.size(); w++) W[w] = add(W[w], part[w]);
        done += cn;
        if (n == 0) break;
    }
    if (want_windows) {
        char* o = reinterpret_cast<char*>(out);
        for (size_t w = 0; w < W.size(); w++) host_store_jac<F>(o + w * sizeof(Jac<F>), W[w]);
    } else {
        host_store_jac<F>(out, host_horner(W.data(), (int)W.size(), c));
    }
    return GA_OK;
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

// ---- MSM ------------------------------------------------------------------------------------------------
int ga_msm(ga_ctx* h, int curve, int group, const void* bases, const void* scalars, size_t n, unsigned flags, void* out_jac) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (!c || !out_jac || (n && (!bases || !scalars))) {
        set_error("ga_msm: null argument");
        return GA_ERR_INVALID;
    }
    Lock l(c);
    return GA_DISPATCH(Scope::G1_FR, curve, group, return (msm_impl<C, G>(c, bases, scalars, n, flags, 0, -1, out_jac, nullptr, nullptr, false)));
} GA_ABI_CATCH

int ga_msm_windows(ga_ctx* h, int curve, int group, const void* bases, const void* scalars, size_t n, unsigned flags, int win_lo,
                   int win_hi, void* out_windows, int* window_bits, int* num_windows) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (!c || !out_windows || (n && (!bases || !scalars))) {
        set_error("ga_msm_windows: null argument");
        return GA_ERR_INVALID;
    }
    Lock l(c);
    return GA_DISPATCH(Scope::G1_FR, curve, group,
                       return (msm_impl<C, G>(c, bases, scalars, n, flags, win_lo, win_hi, out_windows, window_bits, num_windows, true)));
} GA_ABI_CATCH

// ---- fixed-base batch scalar multiplication (fixed_base.hip.h) ---------------------------------------------
int ga_batch_scalar_mul(ga_ctx* h, int curve, int group, const void* base_affine, const void* scalars, size_t n, unsigned flags,
                        void* out_affine) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    constexpr Scope S = Scope::G1_FR;
    GA_CHECK(dispatch_check(S, curve, group));
    if (n == 0) return GA_OK;
    if (!c || !base_affine || !scalars || !out_affine) {
        set_error("ga_batch_scalar_mul: null argument");
        return GA_ERR_INVALID;
    }
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
    if (!window_bits || !num_windows) {
        set_error("ga_batch_scalar_mul_plan: null argument");
        return GA_ERR_INVALID;
    }
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
    if (!c || !powers_affine || !out_affine) {
        set_error("ga_kzg_to_lagrange_g1: null argument");
        return GA_ERR_INVALID;
    }
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
    if (!c || !powers_affine || !out_affine) {
        set_error("ga_lagrange_coeffs: null argument");
        return GA_ERR_INVALID;
    }
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
    if (!c || !points_affine || !scalars || !out_affine) {
        set_error("ga_scale_points: null argument");
        return GA_ERR_INVALID;
    }
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
    if (!out4 || (n > 0 && (!c || !points_affine))) {
        set_error("ga_check_points: null argument");
        return GA_ERR_INVALID;
    }
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
    if (!c || !out2 || (n > 0 && (!p_affine || !q_affine))) {
        set_error("ga_pairing_check: null argument");
        return GA_ERR_INVALID;
    }
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
    if (!c || !row_start || !out_affine || (row_start[n_rows] != 0 && (!points_affine || !terms || !coeffs))) {
        set_error("ga_sparse_point_sums: null argument");
        return GA_ERR_INVALID;
    }
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
    if (!c || !tau || !out) {
        set_error("ga_fr_lagrange_at: null argument");
        return GA_ERR_INVALID;
    }
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
    if (!c || !row_start || !out || (row_start[n_rows] != 0 && (!x || !terms || !coeffs))) {
        set_error("ga_fr_sparse_matvec: null argument");
        return GA_ERR_INVALID;
    }
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
    if (!count) {
        set_error("ga_fr_compact_nonzero: null count");
        return GA_ERR_INVALID;
    }
    if ((uint64_t)n >= (1ull << 31)) {
        set_error("ga_fr_compact_nonzero: n = %zu, at most 2^31 - 1", n);
        return GA_ERR_INVALID;
    }
    if (n == 0) {
        *count = 0;
        return GA_OK;
    }
    if (!c || !v || !out) {
        set_error("ga_fr_compact_nonzero: null argument");
        return GA_ERR_INVALID;
    }
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
    if (!c || !scalars || !out) {
        set_error("ga_fr_powers: null argument");
        return GA_ERR_INVALID;
    }
    Lock l(c);
    return GA_DISPATCH(S, curve, GA_NO_GROUP, return fr_powers_run<C>(c, scalars, first, n, flags, out));
} GA_ABI_CATCH

int ga_msm_plan(int curve, int group, size_t n, int* window_bits, int* num_windows) try {
    GA_ABI_ENTRY();
    return GA_DISPATCH(Scope::G1_FR, curve, group, return msm_plan<C>(G, n, window_bits, num_windows));
} GA_ABI_CATCH

int ga_msm_combine_windows(int curve, int group, const void* windows, int num_windows, int window_bits, void* out_jac) try {
    GA_ABI_ENTRY();
    if (!windows || !out_jac || num_windows <= 0 || window_bits <= 0) {
        set_error("ga_msm_combine_windows: bad argument");
        return GA_ERR_INVALID;
    }
    return GA_DISPATCH(Scope::G1_FR, curve, group, {
        typedef typename GroupField<C, G>::F F;
        std::vector<XYZZ<F>> W(num_windows);
        for (int w = 0; w < num_windows; w++)
            W[w] = host_load_jac<F>(reinterpret_cast<const char*>(windows) + (size_t)w * sizeof(Jac<F>));
        host_store_jac<F>(out_jac, host_horner(W.data(), num_windows, window_bits));
    });
} GA_ABI_CATCH

// ---- precomputed tables ------------------------------------------------------------------------------------
struct MsmTable {
    Ctx* ctx;
    int curve, group, c, nwin;
    size_t n;
    void* d_table;
    uint64_t bytes;
};

int ga_msm_table_create(ga_ctx* h, int curve, int group, const void* bases, size_t n, unsigned flags, ga_msm_table** out) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (!c || !out || !bases || n == 0) {
        set_error("ga_msm_table_create: bad argument");
        return GA_ERR_INVALID;
    }
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
    MsmTable* t = own.t;
    int rc = GA_OK;
    GA_CHECK(GA_DISPATCH(Scope::G1_FR, curve, group, {
        typedef typename GroupField<C, G>::F F;
        rc = msm_plan_table<C>(n, &t->c, &t->nwin, (flags & GA_TABLE_BATCHED) != 0);
        t->bytes = (uint64_t)t->nwin * n * msm_table_point_bytes<C, G>();
        Staged sb{c};
        if (rc == GA_OK) rc = sb.stage(bases, n * sizeof(Affine<F>), flags & GA_BASES_ON_DEVICE);
        if (rc == GA_OK && device_malloc(&t->d_table, t->bytes) != hipSuccess) {
            set_error("ga_msm_table_create: device_malloc(%llu) failed", (unsigned long long)t->bytes);
            rc = GA_ERR_NOMEM;
        }
        if (rc == GA_OK) rc = msm_table_build<C, G>(c, sb.dev, n, t->c, t->d_table);
        if (rc == GA_OK && hipStreamSynchronize(c->stream) != hipSuccess) {
            set_error("ga_msm_table_create: table kernel failed");
            rc = GA_ERR_HIP;
        }
    }));
    if (rc != GA_OK) return rc;
    own.t = nullptr;
    *out = reinterpret_cast<ga_msm_table*>(t);
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

int ga_msm_table_run(ga_msm_table* th, const void* scalars, unsigned flags, void* out_jac) try {
    GA_ABI_ENTRY();
    MsmTable* t = reinterpret_cast<MsmTable*>(th);
    if (!t || !scalars || !out_jac) {
        set_error("ga_msm_table_run: null argument");
        return GA_ERR_INVALID;
    }
    Ctx* c = t->ctx;
    LaneLock l(c);   // a second caller (the PLONK prover commits from several goroutines) runs beside the first on lane 1
    return GA_DISPATCH(Scope::G1_FR, t->curve, t->group, {
        typedef typename GroupField<C, G>::F F;
        Staged ss{c};
        GA_CHECK(ss.stage(scalars, t->n * 32, flags & GA_SCALARS_ON_DEVICE));
        XYZZ<F> sum;
        GA_CHECK((msm_table_device<C, G>(c, t->d_table, ss.dev, t->n, (flags & GA_SCALARS_MONTGOMERY) != 0, t->c, &sum)));
        host_store_jac<F>(out_jac, sum);
    });
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
    Ctx* c = t->ctx;
    LaneLock l(c);   // a second caller (the PLONK prover commits from several goroutines) runs beside the first on lane 1
    return GA_DISPATCH(Scope::G1_FR, t->curve, t->group, {
        typedef typename GroupField<C, G>::F F;
        std::vector<std::unique_ptr<Staged>> st;
        std::vector<const void*> dev(k);
        for (uint32_t j = 0; j < k; j++) {
            st.emplace_back(new Staged{c});
            GA_CHECK(st.back()->stage(scalars[j], t->n * 32, flags & GA_SCALARS_ON_DEVICE));
            dev[j] = st.back()->dev;
        }
        std::vector<XYZZ<F>> sums(k);
        GA_CHECK((msm_table_device_batch<C, G>(c, t->d_table, dev.data(), (int)k, t->n, (flags & GA_SCALARS_MONTGOMERY) != 0,
                                               t->c, sums.data())));
        for (uint32_t j = 0; j < k; j++) host_store_jac<F>((char*)out_jacs + j * sizeof(Jac<F>), sums[j]);
    });
} GA_ABI_CATCH

int ga_msm_table_run_windows(ga_msm_table* th, const void* scalars, unsigned flags, int win_lo, int win_hi, void* out_jac) try {
    GA_ABI_ENTRY();
    MsmTable* t = reinterpret_cast<MsmTable*>(th);
    if (!t || !scalars || !out_jac) {
        set_error("ga_msm_table_run_windows: null argument");
        return GA_ERR_INVALID;
    }
    if (win_lo < 0 || win_hi > t->nwin || win_hi < win_lo) {
        set_error("ga_msm_table_run_windows: window range [%d,%d) outside [0,%d)", win_lo, win_hi, t->nwin);
        return GA_ERR_INVALID;
    }
    Ctx* c = t->ctx;
    LaneLock l(c);   // a second caller (the PLONK prover commits from several goroutines) runs beside the first on lane 1
    return GA_DISPATCH(Scope::G1_FR, t->curve, t->group, {
        typedef typename GroupField<C, G>::F F;
        Staged ss{c};
        GA_CHECK(ss.stage(scalars, t->n * 32, flags & GA_SCALARS_ON_DEVICE));
        XYZZ<F> sum;
        GA_CHECK((msm_table_device<C, G>(c, t->d_table, ss.dev, t->n, (flags & GA_SCALARS_MONTGOMERY) != 0, t->c, &sum, win_lo,
                                         win_hi)));
        host_store_jac<F>(out_jac, sum);
    });
} GA_ABI_CATCH

int ga_fr_linear_combination(ga_ctx* h, int curve, uint64_t n, int k, const void* const* vecs, const void* scalars, void* out,
                             int on_device) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (!c || !vecs || !scalars || (!out && n)) {
        set_error("ga_fr_linear_combination: null argument");
        return GA_ERR_INVALID;
    }
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
    if (!c || (!poly && n) || !point || !value_out) {
        set_error("ga_fr_poly_evaluate: null argument");
        return GA_ERR_INVALID;
    }
    constexpr Scope S = Scope::G1_FR;
    GA_CHECK(dispatch_check(S, curve, GA_NO_GROUP));
    Lock l(c);
    if (n == 0) {
        memset(value_out, 0, 32);
        return GA_OK;
    }
    Staged sp{c};
    GA_CHECK(sp.stage(poly, n * 32, on_device));
    void* q;
    GA_CHECK(c->scratch_get("kzg_quotient", n * 32, &q));
    const uint64_t scan_threads = env_plonk_batch_knobs().scan_threads;
    return GA_DISPATCH(S, curve, GA_NO_GROUP, return kzg_domain_divide<C>(c, sp.dev, n, point, q, value_out, scan_threads));
} GA_ABI_CATCH

// kzg.Open(p, point, pk): claimed value p(point) and the commitment to (p(X) - p(point)) / (X - point) over the pinned SRS
int ga_kzg_open(ga_msm_table* th, const void* poly, size_t n, unsigned flags, const void* point, void* claimed_value_out, void* h_out) try {
    GA_ABI_ENTRY();
    MsmTable* t = reinterpret_cast<MsmTable*>(th);
    if (!t || !poly || !point || !claimed_value_out || !h_out || n == 0) {
        set_error("ga_kzg_open: null argument or empty polynomial");
        return GA_ERR_INVALID;
    }
    if (t->group != GA_G1 || n - 1 > t->n) {
        set_error("ga_kzg_open: the SRS table must be G1 and hold at least len(p) - 1 = %zu points (it has %zu)", n - 1, t->n);
        return GA_ERR_INVALID;
    }
    Ctx* c = t->ctx;
    Lock l(c);
    const uint64_t scan_threads = env_plonk_batch_knobs().scan_threads;
    return GA_DISPATCH(Scope::G1_FR, t->curve, GA_NO_GROUP, {
        typedef typename GroupField<C, GA_G1>::F F;
        Staged sp{c};
        GA_CHECK(sp.stage(poly, n * 32, flags & GA_SCALARS_ON_DEVICE));
        const size_t qn = n > t->n ? n : t->n;
        void* q;
        GA_CHECK(c->scratch_get("kzg_quotient", qn * 32, &q));
        GA_HIP_CHECK(hipMemsetAsync(q, 0, qn * 32, c->stream));
        GA_CHECK(kzg_domain_divide<C>(c, sp.dev, n, point, q, claimed_value_out, scan_threads));
        XYZZ<F> sum;
        GA_CHECK((msm_table_device<C, GA_G1>(c, t->d_table, q, t->n, true, t->c, &sum)));
        host_store_jac<F>(h_out, sum);
    });
} GA_ABI_CATCH

// kzg.Open for `count` polynomials of one length over one SRS: per pass of at most GA_PLONK_BATCH_MAX items the divisions by
// (X - z_j) are one launch chain (plonk_batch.hip.h) and the quotients one batched table MSM
int ga_kzg_open_batch(ga_msm_table* th, const void* const* polys, size_t n, uint32_t count, unsigned flags, const void* points,
                      void* claimed_values_out, void* h_out) try {
    GA_ABI_ENTRY();
    if (count == 0) return GA_OK;
    MsmTable* t = reinterpret_cast<MsmTable*>(th);
    if (!t || !polys || !points || !claimed_values_out || !h_out || n == 0) {
        set_error("ga_kzg_open_batch: null argument or empty polynomial");
        return GA_ERR_INVALID;
    }
    for (uint32_t j = 0; j < count; j++)
        if (!polys[j]) {
            set_error("ga_kzg_open_batch: polys[%u] is null", j);
            return GA_ERR_INVALID;
        }
    if (t->group != GA_G1 || n - 1 > t->n) {
        set_error("ga_kzg_open_batch: the SRS table must be G1 and hold at least len(p) - 1 = %zu points (it has %zu)", n - 1, t->n);
        return GA_ERR_INVALID;
    }
    Ctx* c = t->ctx;
    Lock l(c);
    const PlonkBatchKnobs knobs = env_plonk_batch_knobs();
    uint32_t batch_max = knobs.batch_max;
    while (batch_max > 1 && (uint64_t)batch_max * t->nwin * t->n >= (1ull << 31)) batch_max--;   // the pair index space of one batched MSM
    if ((uint64_t)batch_max * t->nwin * t->n >= (1ull << 31)) {
        set_error("ga_kzg_open_batch: %d windows x %zu points exceed the 2^31 pair index space of the batched table MSM", t->nwin, (size_t)t->n);
        return GA_ERR_INVALID;
    }
    const bool on_device = (flags & GA_SCALARS_ON_DEVICE) != 0;
    const size_t qn = n > t->n ? n : t->n;   // a row of quotients: the table's n scalars (zero beyond the n - 1 coefficients)
    return GA_DISPATCH(Scope::G1_FR, t->curve, GA_NO_GROUP, {
        typedef typename GroupField<C, GA_G1>::F F;
        char *in = nullptr, *q = nullptr, *vals = nullptr;
        auto reserve = [&](uint32_t cnt) -> int {
            GA_CHECK(c->scratch_get("kzg_b_in", on_device ? 256 : (size_t)cnt * n * 32, (void**)&in));
            GA_CHECK(c->scratch_get("kzg_b_quotient", (size_t)cnt * qn * 32, (void**)&q));
            GA_CHECK(c->scratch_get("kzg_b_values", (size_t)cnt * 32, (void**)&vals));
            return GA_OK;
        };
        std::vector<XYZZ<F>> sums(PLONK_BATCH_LIMIT);
        std::vector<uint32_t> stage;   // the division's small upload; read before the MSM of its pass has returned
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
            // the claimed values leave in one copy ahead of the MSM, whose synchronisation (it returns its sums) completes it
            GA_HIP_CHECK(hipMemcpyAsync((char*)claimed_values_out + (size_t)first * 32, vals, (size_t)cnt * 32, hipMemcpyDeviceToHost, c->stream));
            GA_CHECK((msm_table_device_batch<C, GA_G1>(c, t->d_table, dquot, (int)cnt, t->n, true, t->c, sums.data())));
            for (uint32_t j = 0; j < cnt; j++) host_store_jac<F>((char*)h_out + (size_t)(first + j) * sizeof(Jac<F>), sums[j]);
            return GA_OK;
        };
        const int rc = plonk_batch_chunks(count, batch_max, reserve, pass);
        if (rc != GA_OK) {
            hipStreamSynchronize(c->stream);   // `stage` and the caller's polynomials: no copy from them may still be queued
            return rc;
        }
    });
} GA_ABI_CATCH

// ---- host group helpers ---------------------------------------------------------------------------------
int ga_jac_add(int curve, int group, const void* a, const void* b, void* out) try {
    GA_ABI_ENTRY();
    return GA_DISPATCH(Scope::G1_FR, curve, group, {
        typedef typename GroupField<C, G>::F F;
        host_store_jac<F>(out, add(host_load_jac<F>(a), host_load_jac<F>(b)));
    });
} GA_ABI_CATCH

int ga_jac_to_affine(int curve, int group, const void* a, void* out) try {
    GA_ABI_ENTRY();
    return GA_DISPATCH(Scope::G1_FR, curve, group, {
        typedef typename GroupField<C, G>::F F;
        host_store_affine<F>(out, host_load_jac<F>(a));
    });
} GA_ABI_CATCH

int ga_jac_scalar_mul(int curve, int group, const void* a, const void* k, void* out) try {
    GA_ABI_ENTRY();
    return GA_DISPATCH(Scope::G1_FR, curve, group, {
        typedef typename GroupField<C, G>::F F;
        uint32_t kw[8];
        memcpy(kw, k, 32);
        host_store_jac<F>(out, scalar_mul(host_load_jac<F>(a), kw, 8));
    });
} GA_ABI_CATCH

// ---- NTT ------------------------------------------------------------------------------------------------
int ga_domain_create(ga_ctx* h, int curve, uint64_t cardinality, ga_domain** out) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (!c || !out || cardinality == 0) {
        set_error("ga_domain_create: bad argument");
        return GA_ERR_INVALID;
    }
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

int ga_fft(ga_domain* dh, void* data, int direction, int decimation, int on_coset, int on_device) try {
    GA_ABI_ENTRY();
    Domain* d = reinterpret_cast<Domain*>(dh);
    if (!d || !data || (direction != GA_FFT_FORWARD && direction != GA_FFT_INVERSE) || (decimation != GA_DIF && decimation != GA_DIT)) {
        set_error("ga_fft: bad argument");
        return GA_ERR_INVALID;
    }
    Ctx* c = ntt_domain_ctx(d);
    Lock l(c);
    size_t bytes = ntt_domain_size(d) * 32;
    void* dev = data;
    if (!on_device) {
        GA_CHECK(c->scratch_get("fft_io", bytes, &dev));
        GA_HIP_CHECK(hipMemcpyAsync(dev, data, bytes, hipMemcpyHostToDevice, c->stream));
    }
    GA_CHECK(GA_DISPATCH(Scope::G1_FR, ntt_domain_curve(d), GA_NO_GROUP, return ntt_domain_fft<C>(d, dev, direction, decimation, on_coset)));
    if (!on_device) GA_HIP_CHECK(hipMemcpyAsync(data, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    GA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GA_OK;
} GA_ABI_CATCH

// `count` transforms of one size in ONE launch chain (the vector is the grid's y dimension of every pass, ntt.hip.h): what a loop of
// fft.Domain.FFT / FFTInverse over vectors of one domain does (PLONK's L, R, O and h1..h3, prove.go of backend/plonk; the three
// chains of computeH, backend/groth16/bn254/prove.go:362-368).  data = count vectors of `cardinality` elements, contiguous.
int ga_fft_batch(ga_domain* dh, void* data, uint32_t count, int direction, int decimation, int on_coset, int on_device) try {
    GA_ABI_ENTRY();
    if (count == 0) return GA_OK;
    Domain* d = reinterpret_cast<Domain*>(dh);
    if (!d || !data || (direction != GA_FFT_FORWARD && direction != GA_FFT_INVERSE) || (decimation != GA_DIF && decimation != GA_DIT)) {
        set_error("ga_fft_batch: bad argument");
        return GA_ERR_INVALID;
    }
    Ctx* c = ntt_domain_ctx(d);
    Lock l(c);
    const size_t bytes = (size_t)count * ntt_domain_size(d) * 32;
    void* dev = data;
    if (!on_device) {
        GA_CHECK(c->scratch_get("fft_batch_io", bytes, &dev));
        GA_HIP_CHECK(hipMemcpyAsync(dev, data, bytes, hipMemcpyHostToDevice, c->stream));
    }
    GA_CHECK(GA_DISPATCH(Scope::G1_FR, ntt_domain_curve(d), GA_NO_GROUP, return ntt_domain_fft<C>(d, dev, direction, decimation, on_coset, count)));
    if (!on_device) GA_HIP_CHECK(hipMemcpyAsync(data, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    GA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GA_OK;
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
    if (!fx || !in || !h_out) {
        set_error("ga_plonk_quotient_pinned: null argument");
        return GA_ERR_INVALID;
    }
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
    if (!d0 || !lv || !rv || !ov || !permutation || !beta || !gamma || !z_out) {
        set_error("ga_plonk_build_z: null argument");
        return GA_ERR_INVALID;
    }
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
    if (!d0 || !lv || !rv || !ov || !permutation || !betas || !gammas || !z_out) {
        set_error("ga_plonk_build_z_batch: null argument");
        return GA_ERR_INVALID;
    }
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
    if (!fx || !ins || !h_out) {
        set_error("ga_plonk_quotient_pinned_batch: null argument");
        return GA_ERR_INVALID;
    }
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
    if (!d0 || !in || !out) {
        set_error("ga_plonk_vk_create: null argument");
        return GA_ERR_INVALID;
    }
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
    if (!vk || !proofs || !rows_out || !relation_ok) {
        set_error("ga_plonk_verify_scalars: null argument");
        return GA_ERR_INVALID;
    }
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
    if ((flags & GA_PLONK_VERIFY_COMBINED) && !weights) {
        set_error("ga_plonk_verify: GA_PLONK_VERIFY_COMBINED without weights");
        return GA_ERR_INVALID;
    }
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
    if (!c || (!v && n)) {
        set_error("ga_fr_batch_invert: null argument");
        return GA_ERR_INVALID;
    }
    Lock l(c);
    return GA_DISPATCH(Scope::G1_FR, curve, GA_NO_GROUP, return fr_vec_batch_inverse<C>(c, v, n, on_device != 0));
} GA_ABI_CATCH

int ga_compute_h(ga_domain* dh, const void* a, const void* b, const void* cc, uint64_t n_constraints, void* h_out, int on_device) try {
    GA_ABI_ENTRY();
    Domain* d = reinterpret_cast<Domain*>(dh);
    if (!d || !a || !b || !cc || !h_out || n_constraints > ntt_domain_size(d)) {
        set_error("ga_compute_h: bad argument (n_constraints must be <= domain cardinality)");
        return GA_ERR_INVALID;
    }
    Ctx* c = ntt_domain_ctx(d);
    Lock l(c);
    const uint64_t n = ntt_domain_size(d);
    const size_t full = n * 32, part = n_constraints * 32;
    void *da, *db, *dc;
    GA_CHECK(c->scratch_get("compute_h_a", full, &da));
    GA_CHECK(c->scratch_get("compute_h_b", full, &db));
    GA_CHECK(c->scratch_get("compute_h_c", full, &dc));
    const void* src[3] = {a, b, cc};
    void* dst[3] = {da, db, dc};
    for (int k = 0; k < 3; k++) {
        GA_HIP_CHECK(hipMemcpyAsync(dst[k], src[k], part, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
        if (full > part) GA_HIP_CHECK(hipMemsetAsync(reinterpret_cast<char*>(dst[k]) + part, 0, full - part, c->stream));
    }
    GA_CHECK(GA_DISPATCH(Scope::G1_FR, ntt_domain_curve(d), GA_NO_GROUP, return ntt_domain_compute_h<C>(d, da, db, dc)));
    GA_HIP_CHECK(hipMemcpyAsync(h_out, da, full, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    GA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GA_OK;
} GA_ABI_CATCH

// computeH for `count` solutions of one circuit (a loop of prove.go:346-389 over the solutions): every transform is one batched launch
// chain and the point-wise step one launch.  a, b, c = [count][n_constraints] contiguous; h_out = [count][cardinality], bit-reversed.
int ga_compute_h_batch(ga_domain* dh, const void* a, const void* b, const void* cc, uint32_t count, uint64_t n_constraints, void* h_out,
                       int on_device) try {
    GA_ABI_ENTRY();
    if (count == 0) return GA_OK;
    Domain* d = reinterpret_cast<Domain*>(dh);
    if (!d || !a || !b || !cc || !h_out || n_constraints > ntt_domain_size(d)) {
        set_error("ga_compute_h_batch: bad argument (n_constraints must be <= domain cardinality)");
        return GA_ERR_INVALID;
    }
    Ctx* c = ntt_domain_ctx(d);
    Lock l(c);
    const uint64_t n = ntt_domain_size(d);
    const size_t full = n * 32, part = n_constraints * 32;
    void *da, *db, *dc;
    GA_CHECK(c->scratch_get("compute_h_batch_a", (size_t)count * full, &da));
    GA_CHECK(c->scratch_get("compute_h_batch_b", (size_t)count * full, &db));
    GA_CHECK(c->scratch_get("compute_h_batch_c", (size_t)count * full, &dc));
    const void* src[3] = {a, b, cc};
    void* dst[3] = {da, db, dc};
    const hipMemcpyKind in = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    for (int k = 0; k < 3; k++) {
        if (part == full) {
            GA_HIP_CHECK(hipMemcpyAsync(dst[k], src[k], (size_t)count * full, in, c->stream));
        } else if (part) {   // (rows of n_constraints elements into rows of n)
            for (uint32_t j = 0; j < count; j++)
                GA_HIP_CHECK(hipMemcpyAsync((char*)dst[k] + j * full, (const char*)src[k] + j * part, part, in, c->stream));
        }
        GA_CHECK(GA_DISPATCH(Scope::G1_FR, ntt_domain_curve(d), GA_NO_GROUP, return util_pad_fr_batch<C>(c, dst[k], n_constraints, n, count, c->stream)));
    }
    GA_CHECK(GA_DISPATCH(Scope::G1_FR, ntt_domain_curve(d), GA_NO_GROUP, return ntt_domain_compute_h<C>(d, da, db, dc, count)));
    GA_HIP_CHECK(hipMemcpyAsync(h_out, da, (size_t)count * full, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    GA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GA_OK;
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
int ga_gen_bases(ga_ctx* h, int curve, int group, uint64_t seed, size_t n, void* bases_dev, void* dlogs_dev) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    Lock l(c);
    GA_CHECK(GA_DISPATCH(Scope::G1_FR, curve, group, return util_gen_bases<C, G>(c, seed, n, bases_dev, dlogs_dev)));
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
    if (!c || (n && (!a || !b || !out))) {
        set_error("ga_fr_vec_mul: null argument");
        return GA_ERR_INVALID;
    }
    constexpr Scope S = Scope::G1_FR;
    GA_CHECK(dispatch_check(S, curve, GA_NO_GROUP));
    Lock l(c);
    if (n == 0) return GA_OK;
    Staged sa{c}, sb{c};
    GA_CHECK(sa.stage(a, n * 32, on_device));
    GA_CHECK(sb.stage(b, n * 32, on_device));
    void* d_out = out;
    if (!on_device) GA_CHECK(c->scratch_get("fr_vec_out", n * 32, &d_out));
    GA_CHECK(GA_DISPATCH(S, curve, GA_NO_GROUP, return util_fr_vec_mul<C>(c, sa.dev, sb.dev, n, d_out)));
    if (!on_device) GA_HIP_CHECK(hipMemcpyAsync(out, d_out, n * 32, hipMemcpyDeviceToHost, c->stream));
    GA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GA_OK;
} GA_ABI_CATCH

int ga_generator_mul(int curve, int group, const void* k, void* out_jac) try {
    GA_ABI_ENTRY();
    return GA_DISPATCH(Scope::G1_FR, curve, group, {
        typedef typename GroupField<C, G>::F F;
        uint32_t kw[8];
        memcpy(kw, k, 32);
        host_store_jac<F>(out_jac, scalar_mul(to_xyzz(Generator<C, G>::get()), kw, 8));
    });
} GA_ABI_CATCH

int ga_clock_probe(ga_ctx* h, uint32_t micros, double* mhz_out) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (!c || !mhz_out || micros == 0) {
        set_error("ga_clock_probe: bad argument");
        return GA_ERR_INVALID;
    }
    return util_clock_probe(c, micros, mhz_out);   // (no context lock: it is meant to run BESIDE whatever holds it)
} GA_ABI_CATCH

int ga_microbench(ga_ctx* h, char* buf, size_t cap) try {
    GA_ABI_ENTRY();
    Ctx* c = reinterpret_cast<Ctx*>(h);
    Lock l(c);
    return util_microbench(c, buf, cap);
} GA_ABI_CATCH

}  // extern "C"

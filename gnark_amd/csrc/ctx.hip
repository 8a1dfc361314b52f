// The runtime every unit of libgnark_amd.so stands on (declared in common.hip.h): the error store and the exception barrier of the C ABI,
// the entry and lane thread-locals, which (curve, group) pairs are built and the refusal for one that is not, device allocation with
// the HBM reserve, the context's scratch map and the run-time knobs of Tunables.  No entry point and no driver lives here.
#include <stdarg.h>
#include <stdlib.h>

#include <new>

#include "common.hip.h"

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
bool abi_bad_argument(bool bad, const char* what) {
    if (bad) set_error("%s: %s", g_entry, what);
    return bad;
}

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

uint64_t env_u64(const char* name, uint64_t dflt) {
    const char* e = getenv(name);
    return e ? strtoull(e, nullptr, 10) : dflt;
}
int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
int env_flag(const char* name, int dflt) { return env_int(name, dflt) != 0; }
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

}  // namespace ga

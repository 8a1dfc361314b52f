// Groth16 proving key construction, part of the groth16.hip translation unit: the device-resident key (G16Pk: one G16Vec record per base
// vector, indexed by GA_KEY_*, whose `layout` names the path of its MSM) and the guard that counts its users (PkUse); the staged builder
// (G16Stage -> stage_finish -> G16Pk: check, move, domain, gather lists, plan_layouts, build_tables, points); the one-shot key of
// ga_g16_prove_oneshot (its uploader thread) and the key's lifetime.  Key files are read into the same builder by g16_io.hip.h.  The
// drivers of ga_g16_pk_create, ga_g16_builder_* and the layout queries (g16.hip.h) are here, each beside the step it locks.
#pragma once
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "g16.hip.h"

namespace ga {

// dst[idx[i]] = src[i] for elements of `chunks` 16-byte pieces (building the wire-indexed base arrays at pin time)
static __global__ void g16_scatter_points_kernel(u32x4* __restrict__ dst, const u32x4* __restrict__ src, const uint32_t* __restrict__ idx,
                                                 uint64_t n, uint32_t chunks) {
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t i = t / chunks, k = t % chunks;
    if (i >= n) return;
    dst[(uint64_t)idx[i] * chunks + k] = src[i * chunks + k];
}

// One base vector of a key (G1.A, G1.B, G1.Z, G1.K, G2.B: G16Pk::vec[GA_KEY_*]) and the path its MSM takes (vector_msm, groth16.hip).
// Which vectors get a table is decided per vector: when the five tables do not fit the free HBM together (2^26 constraints: 288 GiB),
// the ones that pay most per byte are built -- A, B (G1), K (they share one witness sort), then Z, then the twice as large G2.B -- and
// the rest stay plain (plan_layouts).
struct G16Vec {
    enum Layout {
        PLAIN,           // d = len affine points: an un-pinned MSM (one bucket set per window + Horner)
        COMPACT_TABLE,   // d = windows x len precomputed window multiples (msm_bucket.hip.h): an MSM with its own digits + sort
        // d = windows x nb_wires, laid out by WIRE id with (0,0) at the wires the vector lacks (infinity entries are skipped by the
        // bucket kernel): for a vector that covers (almost) every wire, so that the digit extraction + radix sort of the whole
        // witness is done ONCE and shared by the A, B (G1 and G2) and K MSMs instead of once per filtered copy of the witness
        WIRE_TABLE
    };
    void* d = nullptr;
    uint64_t len = 0, off = 0;       // this key holds points [off, off + len) of the full vector (everything unless sharded by base range)
    // wire id of every point, on the device (the gather lists of prove.go:147-168 for A and B; G2.B refers to G1.B's); K has one only
    // when committed wires are left out (prove.go:231-235; null = W[nbPublic:]), Z none.  The key owns the lists of A, B and K.
    const uint32_t* idx = nullptr;
    int c = 0;                       // window width of the table: the key's c_w when wire-indexed; G2.B's compact table has G1.B's
    Layout layout = PLAIN;
    bool has_table() const { return layout != PLAIN; }
    bool wire_indexed() const { return layout == WIRE_TABLE; }
};

struct G16Pk {
    Ctx* ctx = nullptr;
    int curve = 0;
    uint64_t n = 0;            // domain cardinality
    uint64_t nb_wires = 0;
    Domain* dom = nullptr;
    G16Vec vec[GA_KEY_NB_VECTORS];
    bool any_table() const { return std::any_of(vec, vec + GA_KEY_NB_VECTORS, [](const G16Vec& v) { return v.has_table(); }); }
    bool any_wire_indexed() const { return std::any_of(vec, vec + GA_KEY_NB_VECTORS, [](const G16Vec& v) { return v.wire_indexed(); }); }
    uint64_t len_k_remove = 0;
    std::vector<void*> d_ck_basis, d_ck_sigma;   // pinned pedersen keys (setup.go:260-287, icicle.go:231-261)
    std::vector<uint64_t> ck_len;
    int c_w = 0;   // window width of the wire-indexed tables (one sort of the whole witness serves them all)
    // multi-GPU partition B: this key holds slice [off, off+len) of every base vector (ga_g16_key.shard_index/count)
    uint32_t shard_index = 0, shard_count = 1;
    uint64_t full_len_k = 0;
    // multi-GPU partition A (scalar windows, BASELINE config 4's wording): the WHOLE key is pinned on every device and this one
    // accumulates only share win_index of win_count of the Pippenger windows of every MSM; partial results add up
    uint32_t win_index = 0, win_count = 1;
    uint64_t w_lo = 0, w_hi = 0;   // wire range [w_lo, w_hi) the A and B gather lists (and a filtered K list) of this shard touch
    std::vector<uint8_t> alpha1, beta1, delta1, beta2, delta2;   // affine images (host)
    // fixed-base tables of delta1 / delta2 for the host epilogue: entry [w*15 + d-1] = d * 2^(4w) * delta (XYZZ images), built on first use
    std::once_flag delta_tab_once;
    std::vector<uint8_t> delta1_tab, delta2_tab;
    // In-flight users: every entry point that takes the key holds one PkUse for its whole duration (the host epilogue included,
    // which runs outside the device lock); ga_g16_pk_destroy waits for them, so a caller that frees the key from one thread while
    // another is still proving (Go: `defer pk.FreeGPUResources()` beside a second goroutine's Prove) gets a late free, not a
    // use-after-free.
    std::mutex use_mu;
    std::condition_variable use_cv;
    int users = 0;
    bool dying = false;
    // A key whose base vectors are still ON THEIR WAY (ga_g16_prove_oneshot: the key goes up as plain vectors, is used for ONE proof
    // and dropped -- the Go package's default, PinToGPU = false): an uploader thread copies them in the order the proof consumes
    // them (A, B, K, G2.B, Z) while the proof already runs; an MSM waits for ITS vector (await_vector), not for the key.
    struct Pending {
        std::mutex mu;
        std::condition_variable cv;
        bool done[GA_KEY_NB_VECTORS] = {false, false, false, false, false};
        size_t bytes[GA_KEY_NB_VECTORS] = {0, 0, 0, 0, 0};   // allocation sizes (the buffers go back to the context's spare set)
        // recorded on the uploader's stream behind a vector's copies: the consumer's STREAM waits for it (hipStreamWaitEvent), no host
        // thread does -- a hipStreamSynchronize of the upload stream was seen to return only when another thread's wait for a 54 ms
        // bucket kernel did (profiles/r06_h_oneshot_timeline.txt)
        hipEvent_t ev[GA_KEY_NB_VECTORS] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        ~Pending() {
            for (hipEvent_t e : ev)
                if (e) hipEventDestroy(e);
        }
        int rc = GA_OK;
        std::string err;
        std::thread uploader;
    };
    std::unique_ptr<Pending> pending;
};

struct PkUse {
    G16Pk* pk;
    bool ok = false;
    explicit PkUse(G16Pk* p) : pk(p) {
        if (!pk) return;
        std::lock_guard<std::mutex> g(pk->use_mu);
        if (pk->dying) return;
        pk->users++;
        ok = true;
    }
    ~PkUse() {
        if (!ok) return;
        std::lock_guard<std::mutex> g(pk->use_mu);
        if (--pk->users == 0) pk->use_cv.notify_all();
    }
    PkUse(const PkUse&) = delete;
    PkUse& operator=(const PkUse&) = delete;
};
#define GA_PK_USE(pk)                                                            \
    PkUse _pk_use(pk);                                                           \
    if (!_pk_use.ok) {                                                           \
        set_error("%s: the proving key is being destroyed", current_entry());    \
        return GA_ERR_STATE;                                                     \
    }

// ---- staged key construction (ga_g16_builder_*) -------------------------------------------------------------------------------
// The proving key reaches the device vector by vector, chunk by chunk: every call takes ONE flat pointer to pointer-free memory
// and has copied what it needs when it returns.  This is the shape cgo wants (no Go pointer stored inside a C struct, nothing
// retained after the call) and the shape a streaming reader of the 6-9 GiB key files wants (g16_io.hip.h: ReadDump / ReadFrom feed
// chunks from a pinned staging buffer).  ga_g16_pk_create(struct) is a thin wrapper over it (pk_create_from_struct).
struct G16Stage {
    Ctx* ctx = nullptr;
    int curve = 0;
    uint64_t n = 0, nb_wires = 0;
    uint32_t shard_index = 0, shard_count = 1;
    uint32_t win_index = 0, win_count = 1;
    bool checked = false;                        // ga_g16_pk_read_*_checked: every kept point goes through check_points.hip.h (g16_io.hip.h)
    struct Vec {
        void* d = nullptr;
        uint64_t total = 0, lo = 0, cnt = 0, seen = 0;
        bool reserved = false;
    } v[GA_KEY_NB_VECTORS];
    std::vector<uint8_t> inf[2];                 // InfinityA, InfinityB (Go []bool images)
    bool have_inf[2] = {false, false};
    // the wire ids each mask keeps, ascending (the gather lists of prove.go:147-168): built by a helper thread as soon as a mask is
    // set -- beside the uploads of the vectors, which keep the calling thread busy for 19 ms per GiB -- and joined by stage_finish
    struct WireList {
        std::unique_ptr<uint32_t[]> ids;
        uint64_t size = 0;
        std::thread job;
    } lists[2];
    void start_list(int which) {
        WireList& L = lists[which];
        if (L.job.joinable()) L.job.join();
        L.ids.reset(new uint32_t[inf[which].size() + 8]);   // (uninitialised on purpose: 64 MiB at 2^24 wires)
        L.size = 0;
        const uint8_t* m = inf[which].data();
        const uint64_t nw = inf[which].size();
        uint32_t* out = L.ids.get();
        uint64_t* size = &L.size;
        L.job = std::thread([m, nw, out, size]() {
            uint32_t* p = out;
            uint64_t i = 0;
            for (; i + 8 <= nw; i += 8) {   // masks are zero almost everywhere: eight wires per test
                uint64_t w;
                memcpy(&w, m + i, 8);
                if (w == 0) {
                    for (int k = 0; k < 8; k++) p[k] = (uint32_t)(i + k);
                    p += 8;
                } else {
                    for (int k = 0; k < 8; k++)
                        if (!m[i + k]) *p++ = (uint32_t)(i + k);
                }
            }
            for (; i < nw; i++)
                if (!m[i]) *p++ = (uint32_t)i;
            *size = (uint64_t)(p - out);
        });
    }
    std::vector<uint8_t> pts[GA_KEY_NB_POINTS];  // alpha1, beta1, delta1, beta2, delta2
    std::vector<void*> d_ck_basis, d_ck_sigma;
    std::vector<uint64_t> ck_len;
    std::vector<uint64_t> k_remove;
    std::thread* early_uploader = nullptr;       // one-shot keys: the thread already filling the vectors' buffers (pk_create_from_struct)
    ~G16Stage() {
        for (auto& L : lists)
            if (L.job.joinable()) L.job.join();
        for (auto& x : v) hipFree(x.d);
        for (void* p : d_ck_basis) hipFree(p);
        for (void* p : d_ck_sigma) hipFree(p);
    }
};

// GA_TRACE_PIN=1, process-wide clock: one line per event of a one-shot proof (uploader, waits) on stderr
static void trace_event(const char* what, int arg, double extra_ms = -1.0) {
    static const bool on = getenv("GA_TRACE_PIN") != nullptr;
    static const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    if (!on) return;
    const double t = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (extra_ms >= 0) fprintf(stderr, "[one-shot] %10.2f ms  %s %d (%.2f ms)\n", t, what, arg, extra_ms);
    else fprintf(stderr, "[one-shot] %10.2f ms  %s %d\n", t, what, arg);
}

// the vector `which` of a key is on the device (always true for a key made by ga_g16_pk_create / the builder / a key file)
static int await_vector(G16Pk* pk, int which) {
    G16Pk::Pending* pd = pk->pending.get();
    if (!pd) return GA_OK;
    const auto t0 = std::chrono::steady_clock::now();
    std::unique_lock<std::mutex> g(pd->mu);
    pd->cv.wait(g, [&] { return pd->done[which] || pd->rc != GA_OK; });
    trace_event("MSM waited for vector", which, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    if (pd->rc != GA_OK) {
        set_error("%s", pd->err.c_str());
        return pd->rc;
    }
    g.unlock();
    GA_HIP_CHECK(hipStreamWaitEvent(pk->ctx->work_stream(), pd->ev[which], 0));   // the MSM about to be launched on this lane starts behind the copies
    return GA_OK;
}

// GA_TRACE_PIN=1: milestones of a key's way to the device on stderr (ms since the first mark of the calling thread) -- tools/exp
struct PinTrace {
    bool on;
    std::chrono::steady_clock::time_point t0;
    PinTrace() : on(getenv("GA_TRACE_PIN") != nullptr), t0(std::chrono::steady_clock::now()) {}
    void mark(const char* what) const {
        if (on) fprintf(stderr, "[pin] %8.2f ms  %s\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), what);
    }
};

static int upload(Ctx* ctx, const void* src, size_t bytes, void** dst) {
    *dst = nullptr;
    hipError_t e = device_malloc(dst, bytes ? bytes : 16);
    if (e != hipSuccess) {
        set_error("proving key upload: device_malloc(%zu) failed: %s", bytes, device_malloc_error(e));
        return GA_ERR_NOMEM;
    }
    if (bytes) GA_HIP_CHECK(hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return GA_OK;
}

static void pk_free(G16Pk* pk) {
    if (!pk) return;
    if (pk->pending && pk->pending->uploader.joinable()) pk->pending->uploader.join();   // (it writes into the buffers freed below)
    if (pk->pending && pk->ctx && !pk->any_table()) {   // a one-shot key: its plain vector buffers stay with the context for the next one
        const char* e = getenv("GA_DOMAIN_SPARE");
        Ctx* c = pk->ctx;
        std::lock_guard<std::mutex> g(c->spare_mu);
        if (!(e && atoi(e) == 0) && !c->spare_vectors.have) {
            for (int w = 0; w < GA_KEY_NB_VECTORS; w++) {
                c->spare_vectors.p[w] = pk->vec[w].d;
                c->spare_vectors.bytes[w] = pk->pending->bytes[w];
                pk->vec[w].d = nullptr;
            }
            c->spare_vectors.have = true;
        }
    }
    if (pk->ctx)
        for (const G16Vec& v : pk->vec) pk->ctx->forget_table(v.d);
    for (const G16Vec& v : pk->vec) hipFree(v.d);
    for (int w : {GA_KEY_G1_A, GA_KEY_G1_B, GA_KEY_G1_K}) hipFree(const_cast<uint32_t*>(pk->vec[w].idx));   // (G2.B's is G1.B's)
    for (void* p : pk->d_ck_basis) hipFree(p);
    for (void* p : pk->d_ck_sigma) hipFree(p);
    if (pk->dom) ntt_domain_give_spare(pk->ctx, pk->dom);   // (kept for the next key of this size: common.hip.h)
    delete pk;
}

// waits for every entry point still using the key, then frees it
void pk_destroy(G16Pk* pk) {
    if (!pk) return;
    {   // wait for every entry point still working on this key (provers on other lanes, epilogues outside the device lock)
        std::unique_lock<std::mutex> u(pk->use_mu);
        pk->dying = true;
        pk->use_cv.wait(u, [&] { return pk->users == 0; });
    }
    CtxLock g(pk->ctx);
    for (int l = 0; l < GA_NUM_LANES; l++) hipStreamSynchronize(pk->ctx->lane_stream[l]);
    pk_free(pk);
}

// what a key holds, for callers that orchestrate a sharded proof themselves (gnark_amd/multigpu.py)
int pk_shard_layout(const G16Pk* pk, uint64_t* out8) {
    const G16Vec& z = pk->vec[GA_KEY_G1_Z];   // (win_count: the plain count; which vectors carry tables is pk_table_layout's answer)
    const uint64_t v[8] = {z.off, z.len, pk->w_lo, pk->w_hi, pk->n, pk->nb_wires, pk->win_index, pk->win_count};
    memcpy(out8, v, sizeof v);
    return GA_OK;
}
// out2[0]: which vectors carry a window table (bit GA_KEY_*: 0 G1.A, 1 G1.B, 2 G1.Z, 3 G1.K, 4 G2.B); out2[1]: which of those are laid
// out by wire id over the shared witness sort
int pk_table_layout(const G16Pk* pk, uint64_t* out2) {
    out2[0] = out2[1] = 0;
    for (int w = 0; w < GA_KEY_NB_VECTORS; w++) {
        out2[0] |= (uint64_t)pk->vec[w].has_table() << w;
        out2[1] |= (uint64_t)pk->vec[w].wire_indexed() << w;
    }
    return GA_OK;
}

// ---- the staged builder's steps ------------------------------------------------------------------------------------------------
// (a step that is not static is the driver of its ga_g16_builder_* entry point and takes the context's lock; x_run is that form of a
// step which pk_create_from_struct and the key readers call under the lock they hold)
static int check_shard_index(uint32_t shard_index, uint32_t shard_count) {
    if (shard_index < shard_count) return GA_OK;
    set_error("proving key: shard_index %u >= shard_count %u", shard_index, shard_count);
    return GA_ERR_INVALID;
}
int stage_create(Ctx* ctx, int curve, uint64_t domain_cardinality, uint64_t nb_wires, uint32_t shard_index, uint32_t shard_count, G16Stage** out) {
    if (shard_count == 0) shard_count = 1;
    GA_CHECK(check_shard_index(shard_index, shard_count));
    *out = new G16Stage{ctx, curve, domain_cardinality, nb_wires, shard_index, shard_count};   // (its first six members)
    return GA_OK;
}
void stage_destroy(G16Stage* st) {
    if (!st) return;
    Ctx* ctx = st->ctx;
    CtxLock g(ctx);
    hipStreamSynchronize(ctx->stream);
    delete st;
}
static size_t stage_point_bytes(int curve, int which) {
    const size_t fp = curve == GA_BN254 ? 32 : 48;
    return which == GA_KEY_G2_B ? 4 * fp : 2 * fp;
}
// device bytes of a vector of `len` points (an empty one still gets a buffer; one-shot keys reuse buffers of equal size)
static size_t vector_alloc_bytes(int curve, int which, uint64_t len) {
    return len ? (size_t)len * stage_point_bytes(curve, which) : 16;
}

static int stage_reserve(G16Stage* st, int which, uint64_t total) {
    if (which < 0 || which >= GA_KEY_NB_VECTORS) {
        set_error("proving key: unknown vector id %d", which);
        return GA_ERR_INVALID;
    }
    G16Stage::Vec& x = st->v[which];
    if (x.reserved) {
        set_error("proving key: vector %d reserved twice", which);
        return GA_ERR_STATE;
    }
    const uint64_t base = total / st->shard_count, rem = total % st->shard_count, k = st->shard_index;   // same split as multigpu.shard_range
    x.total = total;
    x.lo = k * base + (k < rem ? k : rem);
    x.cnt = base + (k < rem ? 1 : 0);
    const size_t bytes = vector_alloc_bytes(st->curve, which, x.cnt);
    hipError_t e = device_malloc(&x.d, bytes);
    if (e != hipSuccess) {
        set_error("proving key upload: device_malloc(%zu) failed: %s", bytes, device_malloc_error(e));
        return GA_ERR_NOMEM;
    }
    x.reserved = true;
    return GA_OK;
}
int stage_reserve_run(G16Stage* st, int which, uint64_t total) {
    CtxLock g(st->ctx);
    return stage_reserve(st, which, total);
}

// points [seen, seen + count) of the full vector; only the part inside this shard's range is copied.  `pinned`: the source is
// page-locked memory owned by the caller for the duration of the call (keyio's staging buffers) -- the copy is then truly
// asynchronous and the caller synchronises; otherwise the stream is drained before returning.
static int stage_append(G16Stage* st, int which, const void* points, uint64_t count, bool pinned = false) {
    if (which < 0 || which >= GA_KEY_NB_VECTORS || !st->v[which].reserved) {
        set_error("proving key: append to vector %d before ga_g16_builder_reserve", which);
        return GA_ERR_STATE;
    }
    G16Stage::Vec& x = st->v[which];
    if (x.seen + count > x.total) {
        set_error("proving key: vector %d overflows its reserved length %llu", which, (unsigned long long)x.total);
        return GA_ERR_INVALID;
    }
    const size_t psz = stage_point_bytes(st->curve, which);
    const uint64_t b0 = x.seen > x.lo ? x.seen : x.lo;
    const uint64_t e0 = x.seen + count < x.lo + x.cnt ? x.seen + count : x.lo + x.cnt;
    if (e0 > b0) {
        GA_HIP_CHECK(hipMemcpyAsync((char*)x.d + (b0 - x.lo) * psz, (const char*)points + (b0 - x.seen) * psz, (e0 - b0) * psz,
                                    hipMemcpyHostToDevice, st->ctx->stream));
        if (!pinned) GA_HIP_CHECK(hipStreamSynchronize(st->ctx->stream));   // no host pointer survives this call
    }
    x.seen += count;
    return GA_OK;
}
// the append without a pointer: `count` points that are none of this shard's business
static int stage_skip(G16Stage* st, int which, uint64_t count) {
    if (which < 0 || which >= GA_KEY_NB_VECTORS || !st->v[which].reserved) {
        set_error("%s: skip on vector %d before ga_g16_builder_reserve", current_entry(), which);
        return GA_ERR_STATE;
    }
    G16Stage::Vec& x = st->v[which];
    const bool outside = x.seen + count <= x.lo || x.seen >= x.lo + x.cnt;
    if (!outside || x.seen + count > x.total) {
        set_error("%s: null pointer for points [%llu, %llu) of vector %d, of which this shard keeps [%llu, %llu)", current_entry(),
                  (unsigned long long)x.seen, (unsigned long long)(x.seen + count), which, (unsigned long long)x.lo, (unsigned long long)(x.lo + x.cnt));
        return GA_ERR_INVALID;
    }
    x.seen += count;
    return GA_OK;
}
int stage_append_run(G16Stage* st, int which, const void* points, uint64_t count) {
    CtxLock g(st->ctx);
    return count && !points ? stage_skip(st, which, count) : stage_append(st, which, points, count);
}

// ---- stage_finish: G16Stage -> G16Pk in seven steps, each called once, top to bottom ------------------------------------------------
// 1. what the caller staged is complete and consistent (joins the helper threads that build the gather lists)
static int stage_check(G16Stage* st) {
    for (int w = 0; w < GA_KEY_NB_VECTORS; w++)
        if (!st->v[w].reserved || st->v[w].seen != st->v[w].total) {
            set_error("proving key: vector %d incomplete (%llu of %llu points)", w, (unsigned long long)st->v[w].seen,
                      (unsigned long long)st->v[w].total);
            return GA_ERR_STATE;
        }
    for (int q = 0; q < GA_KEY_NB_POINTS; q++)
        if (st->pts[q].empty()) {
            set_error("proving key: point %d (alpha1, beta1, delta1, beta2, delta2) not set", q);
            return GA_ERR_STATE;
        }
    if (!st->have_inf[0] || !st->have_inf[1]) {
        set_error("proving key: InfinityA / InfinityB not set");
        return GA_ERR_STATE;
    }
    const uint64_t len_a = st->v[GA_KEY_G1_A].total, len_b = st->v[GA_KEY_G1_B].total, len_z = st->v[GA_KEY_G1_Z].total,
                   len_k = st->v[GA_KEY_G1_K].total, len_b2 = st->v[GA_KEY_G2_B].total;
    if (len_z + 1 != st->n) {
        set_error("proving key: len(G1.Z)=%llu but domain cardinality is %llu (expected n-1, setup.go:248-249)",
                  (unsigned long long)len_z, (unsigned long long)st->n);
        return GA_ERR_INVALID;
    }
    if (st->nb_wires >= (1ull << 32)) {
        set_error("proving key: %llu wires exceed the 32-bit wire index space", (unsigned long long)st->nb_wires);
        return GA_ERR_INVALID;
    }
    if (len_a > st->nb_wires || len_b > st->nb_wires || len_k > st->nb_wires || st->k_remove.size() > st->nb_wires ||
        len_k + st->k_remove.size() > st->nb_wires) {   // (nbWires - len(K) - len(k_remove) = nbPublic >= 0; the wire-indexed layouts rely on it)
        set_error("proving key: len(A) %llu, len(B) %llu, len(K) %llu + %zu removed wires do not fit %llu wires", (unsigned long long)len_a,
                  (unsigned long long)len_b, (unsigned long long)len_k, st->k_remove.size(), (unsigned long long)st->nb_wires);
        return GA_ERR_INVALID;
    }
    if (st->inf[0].size() != st->nb_wires || st->inf[1].size() != st->nb_wires) {
        set_error("proving key: InfinityA / InfinityB must have one entry per wire");
        return GA_ERR_INVALID;
    }
    if (st->win_count > 1 && (st->shard_count > 1 || st->win_index >= st->win_count)) {
        set_error("proving key: window sharding (%u of %u) cannot be combined with base-range sharding, and the index must be below the count",
                  st->win_index, st->win_count);
        return GA_ERR_INVALID;
    }
    for (int k = 0; k < 2; k++) {
        if (!st->lists[k].job.joinable()) st->start_list(k);   // (a caller that set the mask through a path without the early start)
        st->lists[k].job.join();
    }
    if (st->lists[0].size != len_a || st->lists[1].size != len_b || len_b2 != len_b) {
        set_error("proving key: InfinityA/B masks disagree with len(A)/len(B), or len(G2.B) != len(G1.B)");
        return GA_ERR_INVALID;
    }
    return GA_OK;
}

// 2. a key that owns the device buffers of this shard's vectors and of the commitment keys
static G16Pk* stage_move(G16Stage* st) {
    G16Pk* pk = new G16Pk();
    pk->ctx = st->ctx;
    pk->curve = st->curve;
    pk->n = st->n;
    pk->nb_wires = st->nb_wires;
    pk->shard_count = st->shard_count;
    pk->shard_index = st->shard_index;
    pk->win_count = st->win_count ? st->win_count : 1;
    pk->win_index = st->win_index;
    for (int w = 0; w < GA_KEY_NB_VECTORS; w++) {
        pk->vec[w].d = st->v[w].d;
        pk->vec[w].len = st->v[w].cnt;
        pk->vec[w].off = st->v[w].lo;
        st->v[w].d = nullptr;
    }
    pk->full_len_k = st->v[GA_KEY_G1_K].total;
    pk->len_k_remove = st->k_remove.size();
    pk->d_ck_basis.swap(st->d_ck_basis);
    pk->d_ck_sigma.swap(st->d_ck_sigma);
    pk->ck_len = st->ck_len;
    return pk;
}

// 4. this shard's slices of the gather lists on the device -- A's and B's from the masks, K's when commitments leave wires out:
//    wireValues[nbPublic:] minus the private committed and commitment wires (prove.go:231-235) -- and the wire range they touch
static int stage_gather_lists(G16Stage* st, G16Pk* pk) {
    Ctx* ctx = st->ctx;
    G16Vec &a = pk->vec[GA_KEY_G1_A], &b = pk->vec[GA_KEY_G1_B], &k = pk->vec[GA_KEY_G1_K];
    uint64_t lo = st->nb_wires, hi = 0;   // the sorted lists are sliced contiguously, so min / max are the slice ends
    auto put = [&](G16Vec& v, const uint32_t* ids) {
        if (v.len) {
            lo = std::min<uint64_t>(lo, ids[v.off]);
            hi = std::max<uint64_t>(hi, (uint64_t)ids[v.off + v.len - 1] + 1);
        }
        void* d = nullptr;
        const int rc = upload(ctx, ids + v.off, v.len * 4, &d);
        v.idx = static_cast<const uint32_t*>(d);
        return rc;
    };
    GA_CHECK(put(a, st->lists[0].ids.get()));
    GA_CHECK(put(b, st->lists[1].ids.get()));
    pk->vec[GA_KEY_G2_B].idx = b.idx;
    std::vector<uint32_t> ik;
    if (const uint64_t nrem = st->k_remove.size()) {
        const uint64_t nb_public = st->nb_wires - pk->full_len_k - nrem;   // (>= 0: stage_check)
        ik.reserve(pk->full_len_k);
        uint64_t j = 0;
        bool ok = true;
        for (uint64_t i = 0; i < nrem; i++)
            ok = ok && st->k_remove[i] >= nb_public && st->k_remove[i] < st->nb_wires && (i == 0 || st->k_remove[i] > st->k_remove[i - 1]);
        for (uint64_t i = nb_public; ok && i < st->nb_wires; i++) {
            if (j < nrem && st->k_remove[j] == i) j++;
            else ik.push_back((uint32_t)i);
        }
        if (!ok || ik.size() != pk->full_len_k) {
            set_error("proving key: k_remove must be strictly increasing wire ids in [nbPublic, nbWires)");
            return GA_ERR_INVALID;
        }
        GA_CHECK(put(k, ik.data()));
    }
    pk->w_lo = st->shard_count == 1 ? 0 : lo;
    pk->w_hi = st->shard_count == 1 ? st->nb_wires : hi;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) {   // no host pointer survives this call
        set_error("proving key upload: stream synchronize failed");
        return GA_ERR_HIP;
    }
    return GA_OK;
}

// Device bytes the tables may take when the caller leaves the choice to the library (precompute = 0) = free HBM - what a single
// caller's proof will allocate on this context (measured: 1.15 KB per constraint at 2^26 with three tables -- sort pairs, task lists,
// hat-domain copies of the plain vectors, input slots, NTT tables --, 1.25 KB allowed, + 10 %) - 4 GiB.  At 2^26 BN254 on an empty
// device: 244 - 88 - 4 = 152 GiB -> A, B, K (144).  Scratch this context already holds (an earlier proof of this size) is credited
// against the allowance: it is not free any more, but it is exactly what the allowance was for.
static double free_table_bytes(Ctx* ctx, uint64_t n) {
    {   // a key that is here to stay: the buffers kept for one-shot keys (6-9 GiB) go back to the device before the tables are sized
        std::lock_guard<std::mutex> g(ctx->spare_mu);
        for (void*& q : ctx->spare_vectors.p) {
            hipFree(q);
            q = nullptr;
        }
        ctx->spare_vectors.have = false;
    }
    size_t free_b = 0, total_b = 0;
    hipMemGetInfo(&free_b, &total_b);
    uint64_t held = 0;
    {
        std::lock_guard<std::mutex> g(ctx->scratch_mu);
        for (const auto& kv : ctx->scratch) held += kv.second.bytes;
    }
    const double per_proof = (double)n * 1280.0;
    const double allowance = per_proof > (double)held ? per_proof - (double)held : 0.0;
    return (double)free_b - 1.1 * allowance - 4.0 * 1073741824.0;
}

// 5. layout and window width of every vector: arithmetic over the lengths, the table entry sizes, `precompute`, the free bytes and the
//    two tunables.  precompute > 0: all five get a table (the caller insists; a table that does not fit fails the call).  precompute
//    == 0: as many as fit the budget, in the order of what a table buys per byte.
struct G16Plan {
    G16Vec::Layout layout[GA_KEY_NB_VECTORS] = {};   // (PLAIN)
    int c[GA_KEY_NB_VECTORS] = {};
    int c_w = 0;
};
// A, B1, K (48 GiB each at 2^26 BN254; with all three the witness is sorted once instead of three times), Z, and last G2.B (twice the
// bytes for the smallest relative gain; it follows G1.B's layout and never gets a table when G1.B, earlier and half as large, did not)
static const int g16_table_preference[GA_KEY_NB_VECTORS] = {GA_KEY_G1_A, GA_KEY_G1_B, GA_KEY_G1_K, GA_KEY_G1_Z, GA_KEY_G2_B};

template <class C>
static int plan_layouts(const G16Pk* pk, int precompute, double free_bytes, int share_pct, uint64_t budget_pct, G16Plan* plan) {
    int nw = 0, own_c[GA_KEY_NB_VECTORS] = {};
    bool ok = msm_plan_table<C>(pk->nb_wires, &plan->c_w, &nw) == GA_OK;
    const uint64_t wide = (uint64_t)nw * pk->nb_wires;   // entries of a wire-indexed table
    for (int w : {GA_KEY_G1_A, GA_KEY_G1_B, GA_KEY_G1_Z, GA_KEY_G1_K}) ok = msm_plan_table<C>(pk->vec[w].len, &own_c[w], &nw) == GA_OK && ok;
    own_c[GA_KEY_G2_B] = own_c[GA_KEY_G1_B];   // (G2.B's compact table is walked with the digits of G1.B's: witness_msms)
    // vectors beyond the table index space (the 2^31 pair space, or a forced GA_TABLE_C too narrow): an error when the caller asked
    // for tables explicitly, otherwise no tables
    if (!ok) return precompute > 0 ? GA_ERR_INVALID : GA_OK;
    // the witness sort is shared between the vectors that cover at least GA_G16_SHARE_MIN_PCT % of the wires (default 90: a sparse
    // vector would make the lanes of the bucket kernel idle on its missing wires, and waste table memory)
    auto dense = [&](uint64_t len) {
        return pk->shard_count == 1 && pk->nb_wires < (1ull << 27) && len > 0 && (double)len * 100.0 >= (double)pk->nb_wires * share_pct;
    };
    const size_t t1 = msm_table_point_bytes<C, GA_G1>(), t2 = msm_table_point_bytes<C, GA_G2>();
    G16Vec::Layout cand[GA_KEY_NB_VECTORS];
    uint64_t bytes[GA_KEY_NB_VECTORS], all_bytes = 0;
    for (int w = 0; w < GA_KEY_NB_VECTORS; w++) {
        const uint64_t len = pk->vec[w].len;   // (len(G2.B) == len(G1.B): stage_check)
        const bool wire = w != GA_KEY_G1_Z && dense(len);
        cand[w] = wire ? G16Vec::WIRE_TABLE : G16Vec::COMPACT_TABLE;
        plan->c[w] = wire ? plan->c_w : own_c[w];
        bytes[w] = (wire ? wide : (own_c[w] > 0 ? (uint64_t)(C::FrP::BITS / own_c[w] + 1) : 0) * len) * (w == GA_KEY_G2_B ? t2 : t1);
        all_bytes += bytes[w];
    }
    double budget = free_bytes;
    if (budget_pct) budget = (double)budget_pct / 100.0 * (double)all_bytes;   // GA_G16_TABLE_BUDGET_PCT (tests: partial tables on small keys)
    for (int w : g16_table_preference) {
        // (the plain array a table replaces is freed once the table stands; while it is built both are resident)
        if (precompute > 0 || (double)bytes[w] <= budget) {
            plan->layout[w] = cand[w];
            budget -= (double)bytes[w];
        } else {
            plan->c[w] = 0;
        }
    }
    return GA_OK;
}

// compact base array -> wire-indexed array with (0,0) at the missing wires; d_idx = the wire id of every entry
static int widen_vector(G16Pk* pk, int which, const uint32_t* d_idx) {
    Ctx* ctx = pk->ctx;
    G16Vec& v = pk->vec[which];
    const size_t psz = stage_point_bytes(pk->curve, which);
    void* wide_arr = nullptr;
    if (device_malloc(&wide_arr, pk->nb_wires * psz) != hipSuccess) {
        set_error("proving key: hipMalloc of a wire-indexed base array failed");
        return GA_ERR_NOMEM;
    }
    hipError_t we = hipMemsetAsync(wide_arr, 0, pk->nb_wires * psz, ctx->stream);
    const uint32_t chunks = (uint32_t)(psz / 16);
    const uint64_t threads = v.len * chunks;
    if (we == hipSuccess) {
        hipLaunchKernelGGL(g16_scatter_points_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream,
                           (u32x4*)wide_arr, (const u32x4*)v.d, d_idx, v.len, chunks);
        we = hipGetLastError();
    }
    if (we == hipSuccess) we = hipStreamSynchronize(ctx->stream);
    if (we != hipSuccess) {
        set_error("proving key: building a wire-indexed base array failed: %s", hipGetErrorString(we));
        hipFree(wide_arr);
        return GA_ERR_HIP;
    }
    hipFree(v.d);
    v.d = wide_arr;
    return GA_OK;
}

// the (compact or widened) base array of a vector -> its table [2^(c*w)]P for every window w (one shared bucket set per MSM afterwards)
template <class C, int G>
static int table_from_vector(G16Pk* pk, int which) {
    Ctx* ctx = pk->ctx;
    G16Vec& v = pk->vec[which];
    const uint64_t rows = v.wire_indexed() ? pk->nb_wires : v.len;
    if (rows == 0) return GA_OK;
    const uint64_t bytes = (uint64_t)(C::FrP::BITS / v.c + 1) * rows * msm_table_point_bytes<C, G>();
    void* t = nullptr;
    if (device_malloc(&t, bytes) != hipSuccess) {
        set_error("proving key: hipMalloc of a %llu-byte window table failed", (unsigned long long)bytes);
        return GA_ERR_NOMEM;
    }
    int r = msm_table_build<C, G>(ctx, v.d, rows, v.c, t);
    if (r == GA_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) r = GA_ERR_HIP;
    hipFree(v.d);
    v.d = t;
    return r;
}

// 6. the plan carried out: the wire-indexed vectors widened (A, B, G2.B, K), then the tables built (A, B, Z, K, G2.B).  A failure
//    leaves a key without tables for pk_free.
template <class C>
static int build_tables(G16Pk* pk, const G16Plan& plan) {
    Ctx* ctx = pk->ctx;
    pk->c_w = plan.c_w;
    for (int w = 0; w < GA_KEY_NB_VECTORS; w++) {
        pk->vec[w].layout = plan.layout[w];
        pk->vec[w].c = plan.c[w];
    }
    if (!pk->any_table()) return GA_OK;
    int rc = GA_OK;
    const G16Vec& k = pk->vec[GA_KEY_G1_K];
    void* d_ik = nullptr;   // wire ids of K's entries when it has no remove-list gather: nbPublic + i
    if (k.wire_indexed() && !k.idx) {
        const uint64_t nbp = pk->nb_wires - k.len;
        std::vector<uint32_t> ikk(k.len);
        for (uint64_t i = 0; i < k.len; i++) ikk[i] = (uint32_t)(nbp + i);
        rc = upload(ctx, ikk.data(), k.len * 4, &d_ik);
        if (rc == GA_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = GA_ERR_HIP;
    }
    for (int w : {GA_KEY_G1_A, GA_KEY_G1_B, GA_KEY_G2_B, GA_KEY_G1_K})
        if (rc == GA_OK && pk->vec[w].wire_indexed()) rc = widen_vector(pk, w, pk->vec[w].idx ? pk->vec[w].idx : static_cast<const uint32_t*>(d_ik));
    hipFree(d_ik);
    for (int w : {GA_KEY_G1_A, GA_KEY_G1_B, GA_KEY_G1_Z, GA_KEY_G1_K, GA_KEY_G2_B})
        if (rc == GA_OK && pk->vec[w].has_table()) rc = w == GA_KEY_G2_B ? table_from_vector<C, GA_G2>(pk, w) : table_from_vector<C, GA_G1>(pk, w);
    if (rc != GA_OK)
        for (G16Vec& v : pk->vec) v.layout = G16Vec::PLAIN;
    return rc;
}

template <class C>
static int stage_finish(G16Stage* st, int precompute, G16Pk** out) {
    Ctx* ctx = st->ctx;
    PinTrace tr;
    GA_CHECK(stage_check(st));                                                      // 1
    tr.mark("finish: gather lists built on the host");
    G16Pk* pk = stage_move(st);                                                     // 2
    pk->dom = ntt_domain_take_spare(ctx, C::ID, pk->n);                             // 3: the domain of the key this context freed last, when it has this size
    int rc = pk->dom ? GA_OK : ntt_domain_new<C>(ctx, pk->n, &pk->dom);
    tr.mark("finish: ntt_domain_new returned");
    if (rc == GA_OK) rc = stage_gather_lists(st, pk);                               // 4
    tr.mark("finish: gather lists uploaded, stream drained");
    if (rc == GA_OK && precompute >= 0) {
        G16Plan plan;
        rc = plan_layouts<C>(pk, precompute, free_table_bytes(ctx, pk->n), ctx->tun.g16_share_min_pct, ctx->tun.g16_table_budget_pct, &plan);   // 5
        if (rc == GA_OK) rc = build_tables<C>(pk, plan);                            // 6
    }
    if (rc != GA_OK) {
        if (st->early_uploader && st->early_uploader->joinable()) st->early_uploader->join();   // (it writes into the buffers pk_free frees)
        pk_free(pk);
        return rc;
    }
    pk->alpha1 = st->pts[GA_KEY_G1_ALPHA];                                          // 7
    pk->beta1 = st->pts[GA_KEY_G1_BETA];
    pk->delta1 = st->pts[GA_KEY_G1_DELTA];
    pk->beta2 = st->pts[GA_KEY_G2_BETA];
    pk->delta2 = st->pts[GA_KEY_G2_DELTA];
    *out = pk;
    return GA_OK;
}

static int stage_set_point(G16Stage* st, int which, const void* affine) {
    if (which < 0 || which >= GA_KEY_NB_POINTS || !affine) {
        set_error("proving key: bad point id %d or null pointer", which);
        return GA_ERR_INVALID;
    }
    const size_t fp = st->curve == GA_BN254 ? 32 : 48;
    const size_t bytes = (which == GA_KEY_G2_BETA || which == GA_KEY_G2_DELTA) ? 4 * fp : 2 * fp;
    st->pts[which].assign((const uint8_t*)affine, (const uint8_t*)affine + bytes);
    return GA_OK;
}
int stage_set_point_run(G16Stage* st, int which, const void* affine) {
    CtxLock g(st->ctx);
    return stage_set_point(st, which, affine);
}

int stage_set_infinity(G16Stage* st, int which, const uint8_t* mask, uint64_t nb_wires) {
    CtxLock g(st->ctx);
    if ((which != 0 && which != 1) || !mask || nb_wires != st->nb_wires) {
        set_error("%s: which must be 0/1 and the mask must have nbWires = %llu entries", current_entry(), (unsigned long long)st->nb_wires);
        return GA_ERR_INVALID;
    }
    if (st->lists[which].job.joinable()) st->lists[which].job.join();   // (a mask set twice: the list of the old one must not outlive it)
    st->inf[which].assign(mask, mask + nb_wires);
    st->have_inf[which] = true;
    st->start_list(which);   // (beside whatever the caller appends next)
    return GA_OK;
}

int stage_set_k_remove(G16Stage* st, const uint64_t* ids, uint64_t len) {
    CtxLock g(st->ctx);
    if (len > st->nb_wires) {
        set_error("%s: %llu removed wires for %llu wires", current_entry(), (unsigned long long)len, (unsigned long long)st->nb_wires);
        return GA_ERR_INVALID;
    }
    st->k_remove.assign(ids, ids + len);
    return GA_OK;
}

int stage_set_window_shard(G16Stage* st, uint32_t index, uint32_t count) {
    CtxLock g(st->ctx);
    if (count == 0 || index >= count) {
        set_error("%s: index %u must be below count %u", current_entry(), index, count);
        return GA_ERR_INVALID;
    }
    st->win_index = index;
    st->win_count = count;
    return GA_OK;
}

static int stage_add_commitment_key(G16Stage* st, const void* basis, const void* sigma, uint64_t len) {
    if (len && (!basis || !sigma)) {
        set_error("proving key: null commitment key basis");
        return GA_ERR_INVALID;
    }
    const size_t s1 = stage_point_bytes(st->curve, GA_KEY_G1_A);
    void *db = nullptr, *ds = nullptr;
    int rc = upload(st->ctx, basis, len * s1, &db);
    if (rc == GA_OK) rc = upload(st->ctx, sigma, len * s1, &ds);
    if (rc == GA_OK && hipStreamSynchronize(st->ctx->stream) != hipSuccess) rc = GA_ERR_HIP;
    if (rc != GA_OK) {
        hipFree(db);
        hipFree(ds);
        return rc;
    }
    st->d_ck_basis.push_back(db);
    st->d_ck_sigma.push_back(ds);
    st->ck_len.push_back(len);
    return GA_OK;
}
int stage_add_commitment_key_run(G16Stage* st, const void* basis, const void* sigma, uint64_t len) {
    CtxLock g(st->ctx);
    return stage_add_commitment_key(st, basis, sigma, len);
}

static int stage_finish_any(G16Stage* st, int precompute, G16Pk** out) {
    return GA_DISPATCH(Scope::FULL, st->curve, GA_NO_GROUP, return stage_finish<C>(st, precompute, out));
}
// ga_g16_builder_finish: the builder is consumed either way, a failed finish leaves nothing half-built behind
int stage_finish_consume(G16Stage* st, int32_t precompute, G16Pk** out) {
    int rc;
    {
        CtxLock g(st->ctx);
        G16Pk* pk = nullptr;
        try {
            rc = stage_finish_any(st, precompute, &pk);
        } catch (const std::exception& e) {   // (host allocations sized by the key: no exception crosses the C ABI)
            set_error("%s: %s", current_entry(), e.what());
            rc = GA_ERR_NOMEM;
        }
        if (rc == GA_OK) *out = pk;
    }
    delete st;
    return rc;
}

// ---- one-shot keys (ga_g16_prove_oneshot) -------------------------------------------------------------------------------------
// the buffers of the previous one-shot key, when they have the sizes this one needs (otherwise they are freed)
static void adopt_spare_vectors(Ctx* ctx, G16Stage* st, const uint64_t* len) {
    std::lock_guard<std::mutex> g(ctx->spare_mu);
    Ctx::SpareVectors& sp = ctx->spare_vectors;
    if (!sp.have) return;
    bool fits = true;
    for (int w = 0; w < GA_KEY_NB_VECTORS; w++) fits = fits && sp.bytes[w] == vector_alloc_bytes(st->curve, w, len[w]);
    for (int w = 0; w < GA_KEY_NB_VECTORS; w++) {
        if (fits) {
            G16Stage::Vec& x = st->v[w];
            x.d = sp.p[w];
            x.total = x.cnt = len[w];
            x.lo = 0;
            x.reserved = true;
        } else {
            hipFree(sp.p[w]);
        }
        sp.p[w] = nullptr;
    }
    sp.have = false;
}

// The uploader thread of a one-shot key, started on the buffers just reserved: the masks, gather lists and domain that
// pk_create_from_struct builds next (30-40 ms at 2^24) are built while the first vector is already on its way.  It copies the
// host vectors of `key` into them in the order the proof consumes them and marks each vector done (await_vector).
static int start_uploader(Ctx* ctx, G16Stage* st, const ga_g16_key* key, G16Pk::Pending* pd) {
    st->early_uploader = &pd->uploader;
    for (int w = 0; w < GA_KEY_NB_VECTORS; w++) {
        pd->bytes[w] = vector_alloc_bytes(key->curve, w, st->v[w].cnt);
        GA_HIP_CHECK(hipEventCreateWithFlags(&pd->ev[w], hipEventDisableTiming));
    }
    // in the order the proof consumes them: A, B, K (G1), B (G2) on the witness lane, Z last (it waits for h anyway)
    struct Job { int which; void* dst; const void* src; size_t bytes; int prio; };
    std::vector<Job> jobs;
    const void* const vec[GA_KEY_NB_VECTORS] = {key->g1_a, key->g1_b, key->g1_z, key->g1_k, key->g2_b};
    int order = 0;
    for (int w : {GA_KEY_G1_A, GA_KEY_G1_B, GA_KEY_G1_K, GA_KEY_G2_B, GA_KEY_G1_Z}) {
        // turn priorities (common.hip.h): W 0 | A 1, B 2 | the solver's A, B, C 3 | K 4, G2.B 5, Z 6.  (K before G2.B, and its MSM
        // before G2.B's in witness_msms: copies make little progress while the G2 bucket kernel runs -- 2 GiB in 72 ms where
        // they take 38 -- so as much as possible is on the device before that kernel starts)
        static const int prio[5] = {1, 2, 4, 5, 6};
        jobs.push_back(Job{w, st->v[w].d, vec[w], (size_t)st->v[w].cnt * stage_point_bytes(key->curve, w), prio[order++]});
    }
    const int device = ctx->device;
    pd->uploader = std::thread([pd, jobs, device, ctx]() {
        int rc = GA_OK;
        std::string err;
        hipStream_t up = nullptr;
        try {
            if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&up, hipStreamNonBlocking) != hipSuccess) {
                rc = GA_ERR_HIP;
                err = "one-shot key upload: no stream";
            }
            for (const Job& j : jobs) {
                if (rc != GA_OK) break;
                hipError_t e = j.bytes ? ctx->h2d_pageable(j.dst, j.src, j.bytes, up, j.prio) : hipSuccess;
                if (e == hipSuccess) e = hipEventRecord(pd->ev[j.which], up);
                std::lock_guard<std::mutex> g(pd->mu);
                if (e != hipSuccess) {
                    rc = GA_ERR_HIP;
                    err = std::string("one-shot key upload: ") + hipGetErrorString(e);
                } else {
                    pd->done[j.which] = true;
                    pd->cv.notify_all();
                    trace_event("uploaded vector", j.which);
                }
            }
        } catch (...) {   // (an exception leaving a thread function terminates the process)
            rc = GA_ERR_STATE;
            err = "one-shot key upload: exception in the uploader thread";
        }
        if (up) {   // the host vectors may be released once this thread has been joined: every copy must have left them
            if (hipStreamSynchronize(up) != hipSuccess && rc == GA_OK) {
                rc = GA_ERR_HIP;
                err = "one-shot key upload: stream synchronize failed";
            }
            hipStreamDestroy(up);
        }
        if (rc != GA_OK) {
            std::lock_guard<std::mutex> g(pd->mu);
            pd->rc = rc;
            pd->err = err;
            pd->cv.notify_all();
        }
    });
    return GA_OK;
}

// the five points, the two masks and every non-empty base vector of a host key description are there
static bool key_points_present(const ga_g16_key* key) {
    return key->g1_alpha && key->g1_beta && key->g1_delta && key->g2_beta && key->g2_delta && key->infinity_a && key->infinity_b &&
           (!key->len_a || key->g1_a) && (!key->len_b || key->g1_b) && (!key->len_z || key->g1_z) && (!key->len_k || key->g1_k) &&
           (!key->len_b2 || key->g2_b);
}

// ga_g16_pk_create: the struct-of-pointers form of the staged builder (C and ctypes callers; from Go only with runtime.Pinner)
// defer_uploads (ga_g16_prove_oneshot): the five base vectors get their device buffers here but are copied by an uploader thread
// that this function starts before it returns -- plain vectors only (no tables), the whole key on one device; the caller must keep
// the host vectors alive until the thread has been joined (pk_free does).
static int pk_create_from_struct(Ctx* ctx, const ga_g16_key* key, G16Pk** out, bool defer_uploads) {
    GA_CHECK(dispatch_check(Scope::FULL, key->curve, GA_NO_GROUP));   // before anything is staged
    if (!key_points_present(key)) {
        set_error("%s: null pointer inside ga_g16_key", current_entry());
        return GA_ERR_INVALID;
    }
    if (key->len_a + key->nb_infinity_a != key->nb_wires || key->len_b + key->nb_infinity_b != key->nb_wires) {
        set_error("proving key: len(A)+NbInfinityA, len(B)+NbInfinityB must equal nbWires and len(G2.B)==len(G1.B)");
        return GA_ERR_INVALID;
    }
    if (key->nb_commitments && (!key->ck_basis || !key->ck_basis_exp_sigma || !key->ck_len)) {
        set_error("proving key: nb_commitments > 0 but the commitment key arrays are null");
        return GA_ERR_INVALID;
    }
    if (key->len_k_remove && !key->k_remove) {
        set_error("proving key: k_remove missing");
        return GA_ERR_INVALID;
    }
    PinTrace tr;
    G16Stage st;
    st.ctx = ctx;
    st.curve = key->curve;
    st.n = key->domain_cardinality;
    st.nb_wires = key->nb_wires;
    st.shard_count = key->shard_count ? key->shard_count : 1;
    st.shard_index = key->shard_index;
    GA_CHECK(check_shard_index(st.shard_index, st.shard_count));
    st.win_count = key->window_shard_count ? key->window_shard_count : 1;
    st.win_index = key->window_shard_index;
    // the masks first: their gather lists are built by helper threads while this thread is busy with the 6-9 GiB of uploads below
    st.inf[0].assign(key->infinity_a, key->infinity_a + key->nb_wires);
    st.inf[1].assign(key->infinity_b, key->infinity_b + key->nb_wires);
    st.have_inf[0] = st.have_inf[1] = true;
    st.start_list(0);
    st.start_list(1);
    const void* vec[GA_KEY_NB_VECTORS] = {key->g1_a, key->g1_b, key->g1_z, key->g1_k, key->g2_b};
    const uint64_t len[GA_KEY_NB_VECTORS] = {key->len_a, key->len_b, key->len_z, key->len_k, key->len_b2};
    if (defer_uploads && (st.shard_count != 1 || st.win_count != 1)) {
        set_error("%s: the key must be whole (no base-range or window sharding)", current_entry());
        return GA_ERR_INVALID;
    }
    if (defer_uploads) adopt_spare_vectors(ctx, &st, len);
    for (int w = 0; w < GA_KEY_NB_VECTORS; w++) {
        if (!st.v[w].reserved) GA_CHECK(stage_reserve(&st, w, len[w]));
        if (defer_uploads) st.v[w].seen = st.v[w].total;   // (the uploader below fills the buffer)
        else GA_CHECK(stage_append(&st, w, vec[w], len[w], /*pinned=*/true));   // one drain below instead of five
        tr.mark("vector reserved + appended");
    }
    GA_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    tr.mark("uploads drained");
    std::unique_ptr<G16Pk::Pending> pending;
    struct JoinOnError {   // an error return below must not free the buffers (G16Stage's destructor) under a running uploader
        G16Pk::Pending* pd = nullptr;
        ~JoinOnError() {
            if (pd && pd->uploader.joinable()) pd->uploader.join();
        }
    } join_on_error;
    if (defer_uploads) {
        pending.reset(new G16Pk::Pending());
        join_on_error.pd = pending.get();
        GA_CHECK(start_uploader(ctx, &st, key, pending.get()));
    }

    const void* pt[GA_KEY_NB_POINTS] = {key->g1_alpha, key->g1_beta, key->g1_delta, key->g2_beta, key->g2_delta};
    for (int q = 0; q < GA_KEY_NB_POINTS; q++) GA_CHECK(stage_set_point(&st, q, pt[q]));
    for (uint32_t i = 0; i < key->nb_commitments; i++) GA_CHECK(stage_add_commitment_key(&st, key->ck_basis[i], key->ck_basis_exp_sigma[i], key->ck_len[i]));
    if (key->len_k_remove) st.k_remove.assign(key->k_remove, key->k_remove + key->len_k_remove);
    tr.mark("points, infinity masks, commitment keys staged");
    G16Pk* pk = nullptr;
    GA_CHECK(stage_finish_any(&st, defer_uploads ? -1 : key->precompute, &pk));
    tr.mark("stage_finish");
    if (defer_uploads) {
        pk->pending = std::move(pending);   // (the key now owns the uploader: pk_free joins it)
        join_on_error.pd = nullptr;
    }
    *out = pk;
    return GA_OK;
}
int pk_create_run(Ctx* ctx, const ga_g16_key* key, G16Pk** out, bool defer_uploads) {
    CtxLock g(ctx);
    return pk_create_from_struct(ctx, key, out, defer_uploads);
}

}  // namespace ga

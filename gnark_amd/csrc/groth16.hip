// Groth16 prover: one-call proof from the solver's output on a device-resident proving key, and the drivers of the proving entry
// points (g16.hip.h; the entry points themselves are g16_abi.hip).  The key (one record per base vector) and its builder are
// g16_key.hip.h, key files and proof bytes are g16_io.hip.h, each with the drivers of its entry points: one translation unit.
//
// Mirrors backend/groth16/bn254/prove.go:130-315 (CPU) and backend/accelerated/icicle/groth16/bn254/icicle.go:784-1360
// (GPU):  computeH -> filter wire values -> 4 G1 MSMs + 1 G2 MSM -> host epilogue with the caller-supplied randomness
// (r, s); BSB22 commitments are the two extra MSMs per commitment of ga_g16_commit (prove.go:84,114) plus the K filter.  The host
// side is C++ because the reference's host side is compiled Go and no Go toolchain exists in the build image (INTEGRATION.md shows
// the cgo binding that calls the entry points).
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "g16_io.hip.h"
#include "g16_key.hip.h"
#include "hostops.hip.h"

namespace ga {

// ---- the device part of a proof, in pieces (a multi-GPU proof runs them on different devices) ----------------------------------
// witness_upload : W -> device, only the wire range this shard's bases cover
// witness_msms   : the schedule of the MSMs over W -- filter, A, B (G1 + G2), K                               prove.go:147-237,283
// vector_msm     : ONE MSM over a base vector of the key, on the path its layout names (wire-indexed table over the shared witness
//                  sort, compact table with its own digits + sort, plain array); k_msm and z_msm feed it K's and Z's scalars
// h_upload       : one of the solver's A, B, C -> device, zero-padded to the domain (h_pad)                      prove.go:356-359
// h_chain        : v <- FFT_coset(iFFT(v)) for one of them (ntt_domain_h_chain)                                prove.go:362-368
// h_combine      : h <- iFFT_coset((a*b - c) * den), bit-reversed like pk.G1.Z (ntt_domain_h_combine)          prove.go:377-386
// z_msm          : MSM over this shard's slice of pk.G1.Z and h                                                prove.go:225-227
// h_side         : the three chains, each once its vector has landed, h_combine and z_msm on ONE lane
// HelperThread   : a thread that runs such pieces beside the caller; its result code, error text and exceptions come back in join()
// prove_batch    : the device part of MANY proofs under one key (ga_g16_prove_batch): chunks of <= 16 solutions, the H side as batched
//                  transforms, one batch MSM per base vector (vector_msm_batch); finish_batch runs the epilogues side by side
// prove_partial runs them on one device (witness_msms on the caller's lane, h_helper beside it), prove_multi / MultiProof on several;
// finish is the host epilogue.  The drivers (g16_*_run, at the end of the file) take the key's use count, the input slot and the locks.

// nbPublic of a proof agrees with the key: nbWires - nbPublic wires feed K, some of them through the commitments' remove list
static int check_nb_public(const G16Pk* pk, uint64_t nb_public) {
    if (nb_public > pk->nb_wires || pk->nb_wires - nb_public != pk->full_len_k + pk->len_k_remove) {
        set_error("prove: inconsistent sizes (nbWires %llu - nbPublic %llu != len(K) %llu + len(k_remove) %llu)", (unsigned long long)pk->nb_wires,
                  (unsigned long long)nb_public, (unsigned long long)pk->full_len_k, (unsigned long long)pk->len_k_remove);
        return GA_ERR_INVALID;
    }
    return GA_OK;
}
// a whole proof needs the whole key
static int check_unsharded(const G16Pk* pk) {
    if (pk->shard_count != 1 || pk->win_count != 1) {
        set_error("%s: this key holds one share of a sharded key (base range %u/%u, windows %u/%u); use ga_g16_prove_multi or "
                  "ga_g16_prove_partial + ga_g16_finish", current_entry(), pk->shard_index, pk->shard_count, pk->win_index, pk->win_count);
        return GA_ERR_STATE;
    }
    return GA_OK;
}
static int check_nb_constraints(const G16Pk* pk, uint64_t n_constraints) {
    if (n_constraints > pk->n) {
        set_error("prove: %llu constraints exceed the domain cardinality %llu", (unsigned long long)n_constraints, (unsigned long long)pk->n);
        return GA_ERR_INVALID;
    }
    return GA_OK;
}

// W -> device, only the wire range this shard reads.  Returns when the copy has been handed to the DMA engine from pageable
// memory, i.e. when the host buffer has been consumed -- callers start the (PCIe-competing) upload of A, B, C only after it.
static int witness_upload(G16Pk* pk, const SlotLease& slot, const void* w, uint64_t nb_public, hipStream_t up_stream = nullptr) {
    Ctx* ctx = pk->ctx;
    GA_CHECK(check_nb_public(pk, nb_public));
    void* d_w;
    GA_CHECK(ctx->scratch_get(slot.name("g16_w").c_str(), pk->nb_wires * 32, &d_w));
    if (!up_stream) up_stream = ctx->work_stream();
    // the wire range this shard reads: everything for an unsharded key, ~1/N of W for shard k of N (the gather lists of a
    // shard are contiguous pieces of the sorted wire lists); K's range depends on nbPublic
    uint64_t lo = pk->w_lo, hi = pk->w_hi;
    const G16Vec& k = pk->vec[GA_KEY_G1_K];
    if (k.len && !k.idx) {
        const uint64_t klo = nb_public + k.off, khi = klo + k.len;
        lo = lo < klo ? lo : klo;
        hi = hi > khi ? hi : khi;
    }
    if (hi > pk->nb_wires) hi = pk->nb_wires;
    if (lo > hi) lo = hi;
    // (timed only on the main stream: a staging thread runs outside the device lock that guards the profiler's stage list)
    StageTimer tm(up_stream == ctx->work_stream() ? ctx : nullptr, "g16_h2d_w", up_stream);
    if (hi > lo) GA_HIP_CHECK(ctx->h2d_pageable((char*)d_w + lo * 32, (const char*)w + lo * 32, (hi - lo) * 32, up_stream, /*prio=*/0));
    return GA_OK;
}

// The four partial sums of a proof before randomisation -- Ar, Bs1, Krs in G1, Bs2 in G2 -- which add up across shards.
// store / load: the ABI's partials image (include/gnark_amd.h, ga_g16_prove_partial): three G1 Jacobians, then one G2 Jacobian.
template <class C>
struct G16Partials {
    typedef Fe<typename C::FpP> F1;
    typedef Fe2<typename C::FpP> F2;
    XYZZ<F1> ar = xyzz_inf<F1>(), bs1 = xyzz_inf<F1>(), krs = xyzz_inf<F1>();
    XYZZ<F2> bs2 = xyzz_inf<F2>();
    void store(void* out) const {
        char* o = reinterpret_cast<char*>(out);
        host_store_jac<F1>(o, ar);
        host_store_jac<F1>(o + sizeof(Jac<F1>), bs1);
        host_store_jac<F1>(o + 2 * sizeof(Jac<F1>), krs);
        host_store_jac<F2>(o + 3 * sizeof(Jac<F1>), bs2);
    }
    void load(const void* in) {
        const char* i = reinterpret_cast<const char*>(in);
        ar = host_load_jac<F1>(i);
        bs1 = host_load_jac<F1>(i + sizeof(Jac<F1>));
        krs = host_load_jac<F1>(i + 2 * sizeof(Jac<F1>));
        bs2 = host_load_jac<F2>(i + 3 * sizeof(Jac<F1>));
    }
};

// What the two halves of a split proof share (prove_partial): the sort of the whole witness, made once on the lane of the
// witness MSMs, and the K MSM, which goes to whichever lane gets to it first.
struct WitnessShared {
    MsmPrepared prep_w;            // digits + sort of W (wire-indexed tables); arrays live in the witness lane's scratch
    bool w_live = false;
    void* d_w = nullptr;           // W on the device (the slot's buffer, in the witness lane's scratch namespace)
    hipEvent_t w_ev = nullptr;     // recorded on the witness lane's stream once W is on the device and prep_w has been launched
    std::mutex mu;
    std::condition_variable cv;
    bool posted = false, failed = false;   // host-side: prep_w / w_ev are valid (or never will be)
    std::atomic<int> k_owner{-1};          // lane that claimed the K MSM
    void post(bool ok) {
        {
            std::lock_guard<std::mutex> g(mu);
            posted = true;
            failed = !ok;
        }
        cv.notify_all();
    }
    bool wait_posted() {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return posted; });
        return !failed;
    }
    bool claim_k(int lane) {
        int expected = -1;
        return k_owner.compare_exchange_strong(expected, lane);
    }
    ~WitnessShared() {
        if (w_ev) hipEventDestroy(w_ev);
    }
};

// digits + sort a compact-table MSM has left in scratch slot 0: the next MSM over the SAME scalars, window width and window share
// (G2.B after G1.B) walks its table with them instead of preparing its own
struct PrepSlot {
    MsmPrepared prep;
    bool live = false;
};

// One MSM over base vector `which` of the key on the calling thread's lane, on the path the vector's layout names:
//   WIRE_TABLE    over `shared_sort`, the digits + sort of the whole witness (null: this device's window share is empty -> infinity)
//   COMPACT_TABLE over the vector's own digits + sort of `scalars` (one per point), made here unless `reuse` holds live ones; they are
//                 left in `reuse`.  An empty vector or an empty window share gives infinity.
//   PLAIN         an un-pinned MSM over `scalars` with the key's window share, once the vector is on the device (await_vector)
template <class C, int G>
static int vector_msm(G16Pk* pk, int which, const void* scalars, const MsmPrepared* shared_sort, PrepSlot* reuse,
                      XYZZ<typename GroupField<C, G>::F>* out) {
    Ctx* ctx = pk->ctx;
    const G16Vec& v = pk->vec[which];
    *out = xyzz_inf<typename GroupField<C, G>::F>();
    switch (v.layout) {
    case G16Vec::WIRE_TABLE:
        return shared_sort ? msm_table_device_reuse<C, G>(ctx, v.d, *shared_sort, out) : GA_OK;
    case G16Vec::COMPACT_TABLE: {
        int lo, hi;
        window_share(C::FrP::BITS / v.c + 1, pk->win_index, pk->win_count, &lo, &hi);
        if (v.len == 0 || hi <= lo) return GA_OK;
        PrepSlot own;
        PrepSlot& p = reuse ? *reuse : own;
        if (!p.live) GA_CHECK(msm_prepare_table_scalars<C>(ctx, scalars, v.len, true, v.c, &p.prep, 0, lo, hi));
        p.live = true;
        return msm_table_device_reuse<C, G>(ctx, v.d, p.prep, out);
    }
    default:
        GA_CHECK(await_vector(pk, which));
        return host_msm<C, G>(ctx, v.d, scalars, v.len, true, out, pk->win_index, pk->win_count);
    }
}

// the K MSM (prove.go:231-237) on the CALLING thread's lane: its scalars are W[nbPublic:], gathered through the remove list when
// commitments leave wires out (scratch of the calling lane); a wire-indexed K needs neither.  `sh` must have been posted.
template <class C>
static int k_msm(G16Pk* pk, uint64_t nb_public, WitnessShared& sh, XYZZ<Fe<typename C::FpP>>* out) {
    Ctx* ctx = pk->ctx;
    const G16Vec& k = pk->vec[GA_KEY_G1_K];
    const void* d_wk = nullptr;
    if (!k.wire_indexed()) {
        void* const d_w = sh.d_w;   // (not scratch_get: the calling thread may be on the partner lane, whose namespace differs)
        d_wk = (const char*)d_w + (nb_public + k.off) * 32;
        if (k.idx) {
            void* g;
            GA_CHECK(ctx->scratch_get("g16_wk", k.len * 32 + 32, &g));
            GA_CHECK(util_gather_fr<C>(ctx, g, d_w, k.idx, k.len));
            d_wk = g;
        }
    }
    return vector_msm<C, GA_G1>(pk, GA_KEY_G1_K, d_wk, sh.w_live ? &sh.prep_w : nullptr, nullptr, out);
}

// The witness MSMs A, B (G1 and G2) and -- unless the partner lane claims it first -- K, on the calling thread's lane, into
// out->ar, bs1, bs2 and (the K sum alone) krs.  `sh` is posted as soon as the shared witness sort has been launched; out->krs is
// written only when *did_k comes back true.  This function is the SCHEDULE; every MSM is a vector_msm.
template <class C>
static int witness_msms(G16Pk* pk, const SlotLease& slot, uint64_t nb_public, WitnessShared& sh, G16Partials<C>* out, bool* did_k) {
    typedef Fe<typename C::FpP> F1;
    Ctx* ctx = pk->ctx;
    const G16Vec &a = pk->vec[GA_KEY_G1_A], &b = pk->vec[GA_KEY_G1_B], &k = pk->vec[GA_KEY_G1_K], &b2 = pk->vec[GA_KEY_G2_B];
    struct PostGuard {   // a failure before the post must still release the partner lane
        WitnessShared& sh;
        bool done = false;
        ~PostGuard() {
            if (!done) sh.post(false);
        }
    } pg{sh};
    *did_k = false;
    GA_CHECK(check_nb_public(pk, nb_public));
    // 1. scratch
    hipStream_t st = ctx->work_stream();
    void *d_w, *d_wa, *d_wb;
    GA_CHECK(ctx->scratch_get(slot.name("g16_w").c_str(), pk->nb_wires * 32, &d_w));
    GA_CHECK(ctx->scratch_get("g16_wa", a.len * 32 + 32, &d_wa));
    GA_CHECK(ctx->scratch_get("g16_wb", b.len * 32 + 32, &d_wb));
    // 2. digits + sort of the WHOLE witness once (scratch slot 1), reused by every wire-indexed table
    if (pk->any_wire_indexed()) {
        int lo, hi;
        window_share(C::FrP::BITS / pk->c_w + 1, pk->win_index, pk->win_count, &lo, &hi);
        if (hi > lo) {
            GA_CHECK(msm_prepare_table_scalars<C>(ctx, d_w, pk->nb_wires, true, pk->c_w, &sh.prep_w, 1, lo, hi));
            sh.w_live = true;
        }
    }
    const MsmPrepared* const shared = sh.w_live ? &sh.prep_w : nullptr;
    // 3. the partner lane may go ahead
    sh.d_w = d_w;
    GA_HIP_CHECK(hipEventRecord(sh.w_ev, st));
    pg.done = true;
    sh.post(true);
    // 4. wire filtering (prove.go:147-168) for the vectors that are not walked by wire id
    if (!a.wire_indexed()) GA_CHECK(util_gather_fr<C>(ctx, d_wa, d_w, a.idx, a.len));
    if (!b.wire_indexed() || !b2.wire_indexed()) GA_CHECK(util_gather_fr<C>(ctx, d_wb, d_w, b.idx, b.len));   // (G2.B may be plain beside a wire-indexed G1.B)
    // 5. The wire-indexed G1 tables (A, B1 and -- when this lane gets it -- K) in ONE pass of the bucket kernel, the merge and the window
    // reduction over the shared witness sort (msm_table_device_reuse_multi): one kernel tail, one reduction with k x the waves and
    // one host synchronisation instead of k of each (prove.go:194,207,237: three MultiExp over the same wireValues).  A table the
    // bucket kernel has found degenerate (a DummySetup key) keeps its own pass with the complete loop; GA_G16_BATCH_TABLES=0: round 5.
    bool in_pass[GA_KEY_NB_VECTORS] = {};
    if (shared && ctx->tun.g16_batch_tables.load(std::memory_order_relaxed)) {
        int who[3], nt = 0;
        const void* tabs[3];
        XYZZ<F1>* dst[3];
        auto fits = [&](const G16Vec& v) { return v.wire_indexed() && !ctx->is_degenerate(v.d); };
        auto join = [&](int which, XYZZ<F1>* sum) {
            who[nt] = which;
            tabs[nt] = pk->vec[which].d;
            dst[nt++] = sum;
        };
        if (fits(a)) join(GA_KEY_G1_A, &out->ar);
        if (fits(b)) join(GA_KEY_G1_B, &out->bs1);
        const bool k_fits = fits(k);
        if (nt + (k_fits ? 1 : 0) >= 2) {
            if (k_fits && sh.claim_k(current_lane())) {
                join(GA_KEY_G1_K, &out->krs);
                *did_k = true;
            }
            if (nt >= 2) {
                XYZZ<F1> sums[3];
                GA_CHECK((msm_table_device_reuse_multi<C, GA_G1>(ctx, tabs, nt, *shared, sums)));
                for (int i = 0; i < nt; i++) *dst[i] = sums[i];
            } else {   // (K went to the partner lane after all: one table left)
                GA_CHECK((vector_msm<C, GA_G1>(pk, who[0], nullptr, shared, nullptr, dst[0])));
            }
            for (int i = 0; i < nt; i++) in_pass[who[i]] = true;
        }
    }
    // 6. A   7. G1.B, which leaves the digits of wB behind when its table is compact
    PrepSlot wb;
    if (!in_pass[GA_KEY_G1_A]) GA_CHECK((vector_msm<C, GA_G1>(pk, GA_KEY_G1_A, d_wa, shared, nullptr, &out->ar)));
    if (!in_pass[GA_KEY_G1_B]) GA_CHECK((vector_msm<C, GA_G1>(pk, GA_KEY_G1_B, d_wb, shared, &wb, &out->bs1)));
    // 8. a key still on its way: K's MSM before G2.B's (upload order)
    if (pk->pending && !*did_k && sh.claim_k(current_lane())) {
        GA_CHECK(k_msm<C>(pk, nb_public, sh, &out->krs));
        *did_k = true;
    }
    // 9. G2.B: the shared witness sort again, or a compact table (window width of G1.B's) walked with the digits G1.B has just made
    GA_CHECK((vector_msm<C, GA_G2>(pk, GA_KEY_G2_B, d_wb, shared, &wb, &out->bs2)));
    // 10. K, unless some lane has it already
    if (!*did_k && sh.claim_k(current_lane())) {
        GA_CHECK(k_msm<C>(pk, nb_public, sh, &out->krs));
        *did_k = true;
    }
    return GA_OK;
}

// ---- the H side -----------------------------------------------------------------------------------------------------------------
// the slot's staging buffer for the solver's A, B or C (k = 0, 1, 2): n elements
static int h_buffer(G16Pk* pk, const SlotLease& slot, int k, void** out) {
    static const char* const names[3] = {"h_a", "h_b", "h_c"};
    return pk->ctx->scratch_get(slot.name(names[k]).c_str(), pk->n * 32, out);
}

// computeH pads to the domain size (prove.go:356-359): rows [n_constraints, n) of d_v <- 0 on `st`
static int h_pad(G16Pk* pk, void* d_v, uint64_t n_constraints, hipStream_t st) {
    if (pk->n > n_constraints) GA_HIP_CHECK(hipMemsetAsync((char*)d_v + n_constraints * 32, 0, (pk->n - n_constraints) * 32, st));
    return GA_OK;
}

// v (host, n_constraints elements) -> device buffer d_v (n elements, zero-padded) on `up_stream`; `landed` (optional) is recorded
// behind it for the stream that consumes d_v
static int h_upload(G16Pk* pk, const void* v, uint64_t n_constraints, void* d_v, hipStream_t up_stream, hipEvent_t landed = nullptr) {
    GA_CHECK(check_nb_constraints(pk, n_constraints));
    GA_HIP_CHECK(pk->ctx->h2d_pageable(d_v, v, n_constraints * 32, up_stream));
    GA_CHECK(h_pad(pk, d_v, n_constraints, up_stream));
    if (landed) GA_HIP_CHECK(hipEventRecord(landed, up_stream));
    return GA_OK;
}

template <class C>
static int z_msm(G16Pk* pk, const void* d_h_slice, XYZZ<Fe<typename C::FpP>>* out) {
    if (pk->vec[GA_KEY_G1_Z].len == 0) {   // (a shard without a slice of Z does not wait for the vector either)
        *out = xyzz_inf<Fe<typename C::FpP>>();
        return GA_OK;
    }
    return vector_msm<C, GA_G1>(pk, GA_KEY_G1_Z, d_h_slice, nullptr, nullptr, out);
}

// The H side of a proof on the calling thread's lane (prove.go:134,346-389, then 225-227): each chain FFT_coset(iFFT(.)) as soon as
// its vector is complete -- landed[k], when given, is waited for on the lane's stream --, the point-wise step and the last transform
// (h in d_h[0], bit-reversed like pk.G1.Z), then the MSM over this key's slice of Z.
template <class C>
static int h_side(G16Pk* pk, void* const d_h[3], const hipEvent_t* landed, XYZZ<Fe<typename C::FpP>>* z_part) {
    hipStream_t st = pk->ctx->work_stream();
    for (int k = 0; k < 3; k++) {
        if (landed) GA_HIP_CHECK(hipStreamWaitEvent(st, landed[k], 0));
        GA_CHECK(ntt_domain_h_chain<C>(pk->dom, d_h[k]));
    }
    GA_CHECK(ntt_domain_h_combine<C>(pk->dom, d_h[0], d_h[1], d_h[2]));
    return z_msm<C>(pk, (const char*)d_h[0] + pk->vec[GA_KEY_G1_Z].off * 32, z_part);
}

// the K MSM on the PARTNER lane, if the witness lane has not got to it yet (its W and its witness sort are on the device: w_ev)
template <class C>
static int k_msm_late(G16Pk* pk, uint64_t nb_public, WitnessShared& sh, XYZZ<Fe<typename C::FpP>>* out, bool* did_k) {
    if (!sh.wait_posted() || !sh.claim_k(current_lane())) return GA_OK;
    GA_HIP_CHECK(hipStreamWaitEvent(pk->ctx->work_stream(), sh.w_ev, 0));
    GA_CHECK(k_msm<C>(pk, nb_public, sh, out));
    *did_k = true;
    return GA_OK;
}

// A helper thread of an entry point.  It runs `body` -- an ordinary function that returns a GA_* code -- on the context's device, on
// `lane`, under the entry-point name of the thread that started it.  No exception leaves the thread function, which would terminate
// the process: it becomes the code abi_exception_code gives it.  join() returns body's code unchanged and republishes its error text
// on the joining thread; the destructor joins, so neither an early return nor an exception on the starting thread leaves a joinable
// std::thread behind.  run_here() takes a body that shares the calling thread through the same wrapper.
class HelperThread {
    std::thread th;
    int rc = GA_OK;
    char err[1024] = "";   // (a fixed buffer: keeping the text of a std::bad_alloc must not allocate)
    template <class F>
    void run(Ctx* ctx, int lane, const char* entry, F& body) noexcept {
        EntryScope under(entry);
        LaneScope on_lane(lane);
        try {
            rc = [&]() -> int {
                GA_HIP_CHECK(hipSetDevice(ctx->device));
                return body();
            }();
        } catch (...) {
            rc = abi_exception_code(entry);
        }
        if (rc != GA_OK) snprintf(err, sizeof(err), "%s", get_error());
    }

public:
    template <class F>
    void start(Ctx* ctx, int lane, F body) {
        const char* entry = current_entry();
        th = std::thread([this, ctx, lane, entry, body]() mutable { run(ctx, lane, entry, body); });
    }
    template <class F>
    void run_here(Ctx* ctx, int lane, F body) {
        run(ctx, lane, current_entry(), body);
    }
    int join() {
        if (th.joinable()) th.join();
        if (rc != GA_OK) set_error("%s", err);
        return rc;
    }
    ~HelperThread() {
        if (th.joinable()) th.join();
    }
};

// all four vectors of a solution into the slot's staging buffers on the slot's own stream (a caller that found the device busy
// with another proof does this while it waits); returns when the copies have completed, so the host buffers are free again
static int preload_solution(G16Pk* pk, const SlotLease& slot, const void* w, const void* a, const void* b, const void* c,
                            uint64_t n_constraints, uint64_t nb_public) {
    hipStream_t st = pk->ctx->slot_stream[slot.slot];
    GA_CHECK(witness_upload(pk, slot, w, nb_public, st));
    const void* src[3] = {a, b, c};
    for (int k = 0; k < 3; k++) {
        void* d;
        GA_CHECK(h_buffer(pk, slot, k, &d));
        GA_CHECK(h_upload(pk, src[k], n_constraints, d, st));
    }
    GA_HIP_CHECK(hipStreamSynchronize(st));
    return GA_OK;
}

// What the two threads of prove_partial share about the H side: the slot's buffers for A, B, C with the events recorded behind
// their uploads, and what the helper thread computed when the proof was split.
template <class C>
struct HShared {
    void* d_h[3];
    hipEvent_t landed[3] = {nullptr, nullptr, nullptr};
    XYZZ<Fe<typename C::FpP>> z_part = xyzz_inf<Fe<typename C::FpP>>(), k_part = z_part;
    bool did_k = false;
    int init(G16Pk* pk, const SlotLease& slot) {
        for (int k = 0; k < 3; k++) {
            GA_CHECK(h_buffer(pk, slot, k, &d_h[k]));
            GA_HIP_CHECK(hipEventCreateWithFlags(&landed[k], hipEventDisableTiming));
        }
        return GA_OK;
    }
    ~HShared() {
        for (hipEvent_t e : landed)
            if (e) hipEventDestroy(e);
    }
};

// The body of prove_partial's helper thread.  src: the solver's A, B, C on the host (null: preloaded), uploaded on the slot's own
// copy stream (two proofs in flight do not queue their uploads).  split: the thread is on the partner lane and runs the H side there,
// then K's MSM.  It returns with the copy stream drained -- no host pointer outlives the call -- and the partner lane idle.
template <class C>
static int h_helper_steps(G16Pk* pk, hipStream_t up, const void* const* src, uint64_t n_constraints, uint64_t nb_public, bool split,
                          WitnessShared& sh, HShared<C>& h) {
    for (int k = 0; src && k < 3; k++) GA_CHECK(h_upload(pk, src[k], n_constraints, h.d_h[k], up, h.landed[k]));
    if (!split) return GA_OK;
    pk->ctx->stat_split++;
    GA_CHECK(h_side<C>(pk, h.d_h, src ? h.landed : nullptr, &h.z_part));
    return k_msm_late<C>(pk, nb_public, sh, &h.k_part, &h.did_k);
}
template <class C>
static int h_helper(G16Pk* pk, const SlotLease& slot, const void* const* src, uint64_t n_constraints, uint64_t nb_public, bool split,
                    WitnessShared& sh, HShared<C>& h) {
    hipStream_t up = pk->ctx->slot_stream[slot.slot];
    const int rc = h_helper_steps<C>(pk, up, src, n_constraints, nb_public, split, sh, h);
    const hipError_t lane_idle = split ? hipStreamSynchronize(pk->ctx->work_stream()) : hipSuccess;   // (z_msm returns synchronised unless this shard's Z slice is empty)
    const hipError_t uploads_done = src ? hipStreamSynchronize(up) : hipSuccess;
    GA_CHECK(rc);
    GA_HIP_CHECK(lane_idle);
    GA_HIP_CHECK(uploads_done);
    return GA_OK;
}

// The device part of a proof on this key's shard: computeH + the five MSMs over the pinned slices.
// Outputs (before randomisation): A-sum, B1-sum, K-sum + Z-sum (G1), B2-sum (G2) -- to be added across shards.
// preloaded: W, A, B, C already sit in the slot's buffers (preload_solution).
//
// Schedule.  The calling thread uploads W and runs the witness MSMs (A, B1, B2) on its own lane.  A helper thread (h_helper) uploads
// A, B, C on the slot's copy stream and -- when the partner lane is free -- also runs the H side there (h_side): each chain as soon
// as its vector has landed, the point-wise step, the last transform, then the Z MSM over h.  The K MSM goes to whichever lane
// reaches it first.  The two halves share the device: the sorts, reduction tails, host round trips and launch gaps of one run under
// the bucket kernels of the other.  Without a partner lane (profiling on, GA_G16_SPLIT=0, or the lane is taken) the helper only
// uploads and the same h_side follows on the caller's lane after the join, as in round 2.  Either half's result code is returned
// verbatim: g16_prove_run's lane-2 fallback keys on GA_ERR_NOMEM.  Everything is joined before this function returns.
template <class C>
static int prove_partial(G16Pk* pk, const SlotLease& slot, bool preloaded, const void* w, const void* a, const void* b, const void* c,
                         uint64_t n_constraints, uint64_t nb_public, G16Partials<C>* out) {
    Ctx* ctx = pk->ctx;
    GA_CHECK(check_nb_constraints(pk, n_constraints));
    HShared<C> h;
    GA_CHECK(h.init(pk, slot));
    WitnessShared sh;
    GA_HIP_CHECK(hipEventCreateWithFlags(&sh.w_ev, hipEventDisableTiming));
    // lanes pair up, (0, 1) and (2, 3): the H side goes to the partner of the caller's lane when that lane is free
    const int lane = current_lane();
    std::unique_lock<std::mutex> partner;
    if (!ctx->profiling && ctx->tun.g16_split && (lane == 0 || lane == 2)) partner = std::unique_lock<std::mutex>(ctx->lane_mu[lane + 1], std::try_to_lock);
    const bool split = partner.owns_lock();
    // W first: the witness MSMs only need W, and the (PCIe-competing) upload of A, B, C starts when this one has been handed over
    if (!preloaded) GA_CHECK(witness_upload(pk, slot, w, nb_public));
    const void* const abc[3] = {a, b, c};
    const void* const* src = preloaded ? nullptr : abc;
    HelperThread helper;
    if (src || split) helper.start(ctx, split ? lane + 1 : lane, [&] { return h_helper<C>(pk, slot, src, n_constraints, nb_public, split, sh, h); });
    bool did_k = false;
    const int w_rc = witness_msms<C>(pk, slot, nb_public, sh, out, &did_k);
    if (w_rc != GA_OK) {   // (the witness side's error is the one reported; the helper is joined on the way out)
        hipStreamSynchronize(ctx->work_stream());
        return w_rc;
    }
    GA_CHECK(helper.join());
    if (!split) GA_CHECK(h_side<C>(pk, h.d_h, src ? h.landed : nullptr, &h.z_part));
    if (!did_k && !h.did_k) {
        set_error("prove: the K MSM was claimed by no lane");
        return GA_ERR_STATE;
    }
    out->krs = add(did_k ? out->krs : h.k_part, h.z_part);
    return GA_OK;
}

// fixed-base scalar multiplication on the host: table[w*15 + d-1] = d * 16^w * P for the 64 4-bit windows of a 256-bit scalar
template <class F>
static void fixed_base_table(const XYZZ<F>& p, std::vector<uint8_t>& blob) {
    blob.resize((size_t)64 * 15 * sizeof(XYZZ<F>));
    XYZZ<F>* t = reinterpret_cast<XYZZ<F>*>(blob.data());
    XYZZ<F> base = p;
    for (int w = 0; w < 64; w++) {
        XYZZ<F> acc = base;
        for (int d = 1; d <= 15; d++) {
            t[w * 15 + d - 1] = acc;
            acc = add(acc, base);
        }
        base = acc;   // 16 * base
    }
}
template <class F>
static XYZZ<F> fixed_base_mul(const std::vector<uint8_t>& blob, const uint32_t* k8) {
    const XYZZ<F>* t = reinterpret_cast<const XYZZ<F>*>(blob.data());
    XYZZ<F> r = xyzz_inf<F>();
    for (int w = 0; w < 64; w++) {
        const uint32_t d = (k8[w / 8] >> (4 * (w % 8))) & 15u;
        if (d) r = add(r, t[w * 15 + d - 1]);
    }
    return r;
}

// Host epilogue with the prover's randomness (prove.go:171-185,199-200,212-214,241-269,287-292) on the SUMMED partials.
template <class C>
static int finish(G16Pk* pk, G16Partials<C> p, const void* r_mont, const void* s_mont, void* proof_out) {
    typedef typename C::FrP FrP;
    typedef Fe<typename C::FpP> F1;
    typedef Fe2<typename C::FpP> F2;
    StageTimer tm(pk->ctx, "g16_epilogue_host");
    Fe<FrP> r, s;
    memcpy(r.l, r_mont, 32);
    memcpy(s.l, s_mont, 32);
    Fe<FrP> kr = neg(mul(r, s));
    Fe<FrP> rc = from_mont(r), sc = from_mont(s), krc = from_mont(kr);
    // [delta]*r, *s, *kr and [delta2]*s are fixed-base: 4-bit windows over a per-key table (63 additions instead of 254 doublings
    // + ~127 additions each; the epilogue sits on the critical path of a single proof: 1.5 -> 0.6 ms)
    std::call_once(pk->delta_tab_once, [&]() {
        fixed_base_table<F1>(host_load_affine<F1>(pk->delta1.data()), pk->delta1_tab);
        fixed_base_table<F2>(host_load_affine<F2>(pk->delta2.data()), pk->delta2_tab);
    });
    XYZZ<F1> d_r = fixed_base_mul<F1>(pk->delta1_tab, rc.l), d_s = fixed_base_mul<F1>(pk->delta1_tab, sc.l), d_kr = fixed_base_mul<F1>(pk->delta1_tab, krc.l);
    p.bs1 = add(add(p.bs1, host_load_affine<F1>(pk->beta1.data())), d_s);
    p.ar = add(add(p.ar, host_load_affine<F1>(pk->alpha1.data())), d_r);
    p.krs = add(p.krs, d_kr);
    p.krs = add(p.krs, scalar_mul2(p.ar, sc.l, p.bs1, rc.l, 8));   // s*Ar + r*Bs1 on one doubling chain
    p.bs2 = add(add(p.bs2, fixed_base_mul<F2>(pk->delta2_tab, sc.l)), host_load_affine<F2>(pk->beta2.data()));
    char* o = reinterpret_cast<char*>(proof_out);
    host_store_affine<F1>(o, p.ar);
    host_store_affine<F2>(o + sizeof(Affine<F1>), p.bs2);
    host_store_affine<F1>(o + sizeof(Affine<F1>) + sizeof(Affine<F2>), p.krs);
    return GA_OK;
}

// ---- a batch of proofs under one key (ga_g16_prove_batch) ----------------------------------------------------------------------
// `count` solutions of one circuit go through the device in chunks of B <= 16.  One chunk, on the caller's lane (lane 0, under the
// device lock; no partner lane, no input slot, no helper thread for device work):
//   1. the chunk's W vectors -> one buffer [B][nb_wires], its A, B, C -> three buffers [B][n], zero-padded (one launch per buffer)
//   2. the H side as BATCHED transforms: three chains, the point-wise step over B * n elements, the last transform -- seven launch
//      chains per chunk instead of seven per solution (at n = 2^10 a launch is ONE workgroup per vector); h lands in [B][n]
//   3. one batch MSM per base vector, by its layout (vector_msm_batch): the B scalar vectors share the sort, the task list and every
//      kernel's tail.  A vector without a table has no batch path and loops vector_msm over the solutions.
// The host epilogues follow outside the device lock, beside each other (finish_batch).

// most solutions one chunk may hold: the batch MSM's 16 (GA_G16_BATCH_MAX lowers it), what keeps every batched MSM's (scalar, window)
// pairs inside the 2^31 index space msm_plan_prepare checks, and what the free HBM holds beside the key -- per solution its inputs,
// (nb_wires + 3n) x 32 B, the gathered scalar vectors, and the MSM scratch (pairs twice over, keys and values, and the task lists:
// ~24 B per pair of the largest MSM).  Scratch the lane holds already is reused, so it counts as free.  At least 1.
template <class C>
static uint32_t batch_chunk_limit(G16Pk* pk) {
    Ctx* ctx = pk->ctx;
    uint64_t B = (uint64_t)std::max(1, std::min(16, ctx->tun.g16_batch_max.load(std::memory_order_relaxed)));
    uint64_t max_pairs = 0, gathered = 0;
    auto pairs = [&](int c, uint64_t len) {
        if (len == 0 || c <= 0) return;
        const uint64_t per = (uint64_t)(C::FrP::BITS / c + 1) * len;
        max_pairs = std::max(max_pairs, per);
        B = std::min(B, std::max<uint64_t>(1, ((1ull << 31) - 1) / per));
    };
    if (pk->any_wire_indexed()) pairs(pk->c_w, pk->nb_wires);
    for (int w = 0; w < GA_KEY_NB_VECTORS; w++) {
        const G16Vec& v = pk->vec[w];
        if (v.layout == G16Vec::COMPACT_TABLE) pairs(v.c, v.len);
        if (!v.wire_indexed() && w != GA_KEY_G1_Z && w != GA_KEY_G2_B) gathered += v.len;
    }
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
        (void)hipGetLastError();
        return (uint32_t)B;
    }
    uint64_t avail = free_b;
    {
        std::lock_guard<std::mutex> g(ctx->scratch_mu);
        for (const auto& kv : ctx->scratch)
            if (kv.second.lane == 0) avail += kv.second.bytes;
    }
    const uint64_t per_solution = (pk->nb_wires + 3 * pk->n + gathered) * 32 + max_pairs * 24;
    B = std::min(B, std::max<uint64_t>(1, avail / 2 / std::max<uint64_t>(per_solution, 1)));
    return (uint32_t)B;
}

// The MSMs over base vector `which` for the B solutions of a chunk, into out[0..B): solution j's scalars are the v.len (wire-indexed:
// nb_wires) elements at d_scalars + j * stride elements.
//   WIRE_TABLE    the table walks `shared_sort`, the digits + sort of the B witnesses, made once per chunk
//   COMPACT_TABLE one batch MSM over the B scalar vectors (what msm_table_device_batch does); the prepared digits stay in `reuse`,
//                 and a vector that finds live ones of its own width and length there (G2.B after G1.B) walks its table with them
//   PLAIN         no batch path exists for raw bases: vector_msm per solution
template <class C, int G>
static int vector_msm_batch(G16Pk* pk, int which, uint32_t B, const void* d_scalars, uint64_t stride, const MsmPrepared* shared_sort,
                            PrepSlot* reuse, XYZZ<typename GroupField<C, G>::F>* out) {
    Ctx* ctx = pk->ctx;
    const G16Vec& v = pk->vec[which];
    for (uint32_t j = 0; j < B; j++) out[j] = xyzz_inf<typename GroupField<C, G>::F>();
    switch (v.layout) {
    case G16Vec::WIRE_TABLE:
        return shared_sort ? msm_table_device_reuse<C, G>(ctx, v.d, *shared_sort, out) : GA_OK;
    case G16Vec::COMPACT_TABLE: {
        if (v.len == 0) return GA_OK;
        PrepSlot own;
        PrepSlot& p = reuse ? *reuse : own;
        if (!(p.live && p.prep.c == v.c && p.prep.n == v.len && p.prep.nsets == (int)B)) {
            std::vector<const void*> ptrs(B);
            for (uint32_t j = 0; j < B; j++) ptrs[j] = (const char*)d_scalars + (uint64_t)j * stride * 32;
            p.live = false;
            GA_CHECK(msm_prepare_table_scalars<C>(ctx, B == 1 ? ptrs[0] : (const void*)ptrs.data(), v.len, true, v.c, &p.prep, 0, 0, -1, (int)B));
            p.live = true;
        }
        return msm_table_device_reuse<C, G>(ctx, v.d, p.prep, out);
    }
    default:
        for (uint32_t j = 0; j < B; j++)
            GA_CHECK((vector_msm<C, G>(pk, which, (const char*)d_scalars + (uint64_t)j * stride * 32, nullptr, nullptr, &out[j])));
        return GA_OK;
    }
}

// one chunk of B <= 16 solutions: the schedule above.  GA_ERR_NOMEM when the chunk's scratch does not fit (the caller halves B).
template <class C>
static int prove_batch_chunk(G16Pk* pk, uint32_t B, const void* const* w, const void* const* a, const void* const* b, const void* const* c,
                             uint64_t n_constraints, uint64_t nb_public, G16Partials<C>* out) {
    typedef Fe<typename C::FpP> F1;
    typedef Fe2<typename C::FpP> F2;
    Ctx* ctx = pk->ctx;
    hipStream_t st = ctx->work_stream();
    const G16Vec &va = pk->vec[GA_KEY_G1_A], &vb = pk->vec[GA_KEY_G1_B], &vk = pk->vec[GA_KEY_G1_K], &vb2 = pk->vec[GA_KEY_G2_B],
                 &vz = pk->vec[GA_KEY_G1_Z];
    const uint64_t nw = pk->nb_wires, n = pk->n;
    // 1. inputs (scratch names of the batch path's own: the input slots belong to ga_g16_prove's callers)
    void *d_w, *d_h[3];
    GA_CHECK(ctx->scratch_get("g16b_w", (size_t)B * nw * 32 + 32, &d_w));
    static const char* const h_names[3] = {"g16b_a", "g16b_b", "g16b_c"};
    for (int k = 0; k < 3; k++) GA_CHECK(ctx->scratch_get(h_names[k], (size_t)B * n * 32, &d_h[k]));
    {
        StageTimer tm(ctx, "g16_h2d_batch");
        const void* const* src[3] = {a, b, c};
        for (uint32_t j = 0; j < B; j++)
            if (nw) GA_HIP_CHECK(ctx->h2d_pageable((char*)d_w + (uint64_t)j * nw * 32, w[j], nw * 32, st, /*prio=*/0));
        for (int k = 0; k < 3; k++) {
            for (uint32_t j = 0; j < B; j++)
                if (n_constraints) GA_HIP_CHECK(ctx->h2d_pageable((char*)d_h[k] + (uint64_t)j * n * 32, src[k][j], n_constraints * 32, st));
            GA_CHECK(util_pad_fr_batch<C>(ctx, d_h[k], n_constraints, n, B, st));
        }
    }
    // 2. the H side (prove.go:346-389 for every solution): h in d_h[0], [B][n], bit-reversed like pk.G1.Z
    for (int k = 0; k < 3; k++) GA_CHECK(ntt_domain_h_chain<C>(pk->dom, d_h[k], B));
    GA_CHECK(ntt_domain_h_combine<C>(pk->dom, d_h[0], d_h[1], d_h[2], B));
    // 3. the MSMs.  Digits + sort of the B witnesses once (scratch set 1), walked by every wire-indexed table
    MsmPrepared prep_w;
    const MsmPrepared* shared = nullptr;
    if (pk->any_wire_indexed() && nw) {
        std::vector<const void*> ptrs(B);
        for (uint32_t j = 0; j < B; j++) ptrs[j] = (const char*)d_w + (uint64_t)j * nw * 32;
        GA_CHECK(msm_prepare_table_scalars<C>(ctx, B == 1 ? ptrs[0] : (const void*)ptrs.data(), nw, true, pk->c_w, &prep_w, 1, 0, -1, (int)B));
        shared = &prep_w;
    }
    // wire filtering (prove.go:147-168) of the B witnesses for the vectors that are not walked by wire id; K's scalars are W[nbPublic:],
    // gathered through the remove list when commitments leave wires out (prove.go:231-235)
    void *d_wa = nullptr, *d_wb = nullptr;
    const void* d_wk = (const char*)d_w + (nb_public + vk.off) * 32;
    uint64_t k_stride = nw;
    if (!va.wire_indexed()) {
        GA_CHECK(ctx->scratch_get("g16b_wa", (size_t)B * va.len * 32 + 32, &d_wa));
        GA_CHECK(util_gather_fr_batch<C>(ctx, d_wa, d_w, va.idx, va.len, B, va.len, nw));
    }
    if (!vb.wire_indexed() || !vb2.wire_indexed()) {
        GA_CHECK(ctx->scratch_get("g16b_wb", (size_t)B * vb.len * 32 + 32, &d_wb));
        GA_CHECK(util_gather_fr_batch<C>(ctx, d_wb, d_w, vb.idx, vb.len, B, vb.len, nw));
    }
    if (!vk.wire_indexed() && vk.idx) {
        void* g;
        GA_CHECK(ctx->scratch_get("g16b_wk", (size_t)B * vk.len * 32 + 32, &g));
        GA_CHECK(util_gather_fr_batch<C>(ctx, g, d_w, vk.idx, vk.len, B, vk.len, nw));
        d_wk = g;
        k_stride = vk.len;
    }
    std::vector<XYZZ<F1>> s1(B), sz(B);
    std::vector<XYZZ<F2>> s2(B);
    PrepSlot wb;   // G1.B's digits, for G2.B
    GA_CHECK((vector_msm_batch<C, GA_G1>(pk, GA_KEY_G1_A, B, d_wa, va.len, shared, nullptr, s1.data())));
    for (uint32_t j = 0; j < B; j++) out[j].ar = s1[j];
    GA_CHECK((vector_msm_batch<C, GA_G1>(pk, GA_KEY_G1_B, B, d_wb, vb.len, shared, &wb, s1.data())));
    for (uint32_t j = 0; j < B; j++) out[j].bs1 = s1[j];
    GA_CHECK((vector_msm_batch<C, GA_G2>(pk, GA_KEY_G2_B, B, d_wb, vb.len, shared, &wb, s2.data())));
    for (uint32_t j = 0; j < B; j++) out[j].bs2 = s2[j];
    GA_CHECK((vector_msm_batch<C, GA_G1>(pk, GA_KEY_G1_K, B, d_wk, k_stride, shared, nullptr, s1.data())));
    for (uint32_t j = 0; j < B; j++) sz[j] = xyzz_inf<F1>();
    if (vz.len) GA_CHECK((vector_msm_batch<C, GA_G1>(pk, GA_KEY_G1_Z, B, (const char*)d_h[0] + vz.off * 32, n, nullptr, nullptr, sz.data())));
    for (uint32_t j = 0; j < B; j++) out[j].krs = add(s1[j], sz[j]);
    GA_HIP_CHECK(hipStreamSynchronize(st));   // (every MSM returns synchronised; a chunk whose vectors are all empty has only copies in flight)
    return GA_OK;
}

// the device part of `count` proofs: chunks of at most batch_chunk_limit solutions; a chunk of more than one solution that does not
// get its scratch is halved and tried again, GA_ERR_NOMEM is returned for a chunk of one only
template <class C>
static int prove_batch(G16Pk* pk, uint32_t count, const void* const* w, const void* const* a, const void* const* b, const void* const* c,
                       uint64_t n_constraints, uint64_t nb_public, G16Partials<C>* partials) {
    Ctx* ctx = pk->ctx;
    uint32_t B = batch_chunk_limit<C>(pk);
    for (uint32_t done = 0; done < count;) {
        const uint32_t cur = std::min(B, count - done);
        const int rc = prove_batch_chunk<C>(pk, cur, w + done, a + done, b + done, c + done, n_constraints, nb_public, partials + done);
        if (rc != GA_OK) {
            hipStreamSynchronize(ctx->work_stream());   // nothing of the failed chunk is in flight when it is tried again or given up
            if (rc != GA_ERR_NOMEM || cur == 1) return rc;
            B = cur / 2;
            continue;
        }
        done += cur;
    }
    return GA_OK;
}

// The host epilogues of a batch (finish, ~0.6 ms of host arithmetic each) beside each other on min(count, 8) threads, the caller's
// among them: thread t takes proofs t, t + T, ...  They run outside the device lock and touch no device; the threads carry lane 1's
// number only so that finish's stage timer, which belongs to lane 0 and the device lock, stays out of it.  serial (the profiler is
// on and the caller still holds the device lock): one after the other on the calling thread, recorded as stages.
template <class C>
static int finish_batch(G16Pk* pk, const std::vector<G16Partials<C>>& parts, const void* r, const void* s, void* proofs_out, bool serial) {
    typedef Fe<typename C::FpP> F1;
    typedef Fe2<typename C::FpP> F2;
    const uint32_t count = (uint32_t)parts.size();
    const size_t proof_bytes = 2 * sizeof(Affine<F1>) + sizeof(Affine<F2>);
    const uint32_t T = serial ? 1u : std::min<uint32_t>(count, 8u);
    auto share = [&](uint32_t t) -> int {
        for (uint32_t j = t; j < count; j += T)
            GA_CHECK(finish<C>(pk, parts[j], (const char*)r + (size_t)j * 32, (const char*)s + (size_t)j * 32, (char*)proofs_out + (size_t)j * proof_bytes));
        return GA_OK;
    };
    if (serial) return share(0);
    std::vector<HelperThread> threads(T);
    for (uint32_t t = 1; t < T; t++) threads[t].start(pk->ctx, 1, [&share, t] { return share(t); });
    threads[0].run_here(pk->ctx, 1, [&share] { return share(0); });
    int rc = GA_OK;
    for (uint32_t t = T; t-- > 0;) {
        const int rc_t = threads[t].join();
        if (rc_t != GA_OK) rc = rc_t;
    }
    return rc;
}

// BSB22: commitment_i = <values, Basis_i> (pedersen Commit, prove.go:84) and its proof of knowledge <values, BasisExpSigma_i>
// (ProveKnowledge, prove.go:114) -- the ICICLE prover's two commitment MSM blocks (icicle.go:834-873,904-944) in one call.
template <class C>
static int commit(G16Pk* pk, uint32_t index, const void* values, uint64_t n_values, void* commitment_out, void* pok_out) {
    typedef Fe<typename C::FpP> F1;
    Ctx* ctx = pk->ctx;
    if (index >= pk->ck_len.size() || n_values != pk->ck_len[index]) {
        set_error("commit: commitment %u of %zu, %llu values for a basis of %llu points", index, pk->ck_len.size(),
                  (unsigned long long)n_values, (unsigned long long)(index < pk->ck_len.size() ? pk->ck_len[index] : 0));
        return GA_ERR_INVALID;
    }
    XYZZ<F1> com = xyzz_inf<F1>(), pok = xyzz_inf<F1>();
    if (n_values) {
        void* d_v;
        GA_CHECK(ctx->scratch_get("g16_commit_values", n_values * 32, &d_v));
        GA_HIP_CHECK(hipMemcpyAsync(d_v, values, n_values * 32, hipMemcpyHostToDevice, ctx->stream));
        GA_CHECK((host_msm<C, GA_G1>(ctx, pk->d_ck_basis[index], d_v, n_values, true, &com)));
        GA_CHECK((host_msm<C, GA_G1>(ctx, pk->d_ck_sigma[index], d_v, n_values, true, &pok)));
    }
    host_store_affine<F1>(commitment_out, com);
    host_store_affine<F1>(pok_out, pok);
    return GA_OK;
}

// sum_i challenge^i * poks[i]  (Horner from the last point)
template <class C>
static int fold_pok(const void* poks, uint64_t n, const void* challenge_mont, void* out) {
    typedef Fe<typename C::FpP> F1;
    uint32_t ch[8];
    host_fr_canonical<typename C::FrP>(challenge_mont, ch);
    XYZZ<F1> acc = xyzz_inf<F1>();
    for (uint64_t i = n; i-- > 0;) {
        acc = scalar_mul(acc, ch, 8);
        acc = add(acc, host_load_affine<F1>((const char*)poks + i * sizeof(Affine<F1>)));
    }
    host_store_affine<F1>(out, acc);
    return GA_OK;
}
// One proof over several devices from ONE process: keys[i] = shard i of n of the same proving key, each in a context on its own
// device.  One host thread per device for the MSMs plus one for the H side (second lane of the context); the three chains of computeH
// run on the first three devices beside their witness MSMs (with n >= 3 every device uploads 1/n of A, B, C over its own PCIe link and
// forwards the rows to the chain owners over xGMI), b and c travel to device 0 (hipMemcpyPeerAsync), device 0 finishes h and sends
// every device its slice; partial sums are added on the host.  With n = 1 this is ga_g16_prove.
struct MultiShared {
    const uint32_t n;   // threads that meet at each barrier
    std::mutex mu;
    std::condition_variable cv;
    int arrived[4] = {0, 0, 0, 0};
    bool failed = false;
    void fail() {
        std::lock_guard<std::mutex> g(mu);
        failed = true;
        cv.notify_all();
    }
    // all n threads meet here; returns false when some thread failed (everyone then unwinds, the failed thread reports)
    bool barrier(int k) {
        std::unique_lock<std::mutex> g(mu);
        arrived[k]++;
        cv.notify_all();
        cv.wait(g, [&] { return failed || arrived[k] == (int)n; });
        return !failed;
    }
};

// The state of one multi-device proof and the bodies of its threads, all HelperThreads: worker(t) for device t (worker 0 on the
// calling thread) and h_helper(t) beside it.  A thread that leaves early -- an error code or an exception -- releases both sets of
// barriers (Release): the others unwind with GA_OK and are joined, the one that failed returns its own code.
template <class C>
struct MultiProof {
    typedef Fe<typename C::FpP> F1;
    G16Pk* const* pks;
    const uint32_t n;
    const void* w;
    const void* src[3];   // the solver's A, B, C
    const uint64_t n_constraints, nb_public;
    const uint32_t owner[3] = {0, n >= 2 ? 1u : 0u, n >= 3 ? 2u : 0u};   // which device runs which chain: a on 0, b on 1 (or 0), c on 2 (or 0)
    const bool sliced = n >= 3;                                          // three or more devices: no PCIe link carries a whole vector
    const uint64_t cshare = (n_constraints + n - 1) / n;                 // rows of A, B, C per device then
    void* chain_buf[3] = {nullptr, nullptr, nullptr};                    // on the owner's device
    void* dev0_buf[3] = {nullptr, nullptr, nullptr};                     // on device 0
    std::vector<void*> h_slice = std::vector<void*>(n, nullptr);
    std::vector<G16Partials<C>> parts = std::vector<G16Partials<C>>(n);   // per device; the Z sum is added into krs
    MultiShared sh{n}, hs{n};                                            // sh: the device workers; hs: their H-side helper threads
    struct Release {
        MultiProof& p;
        bool done = false;
        ~Release() {
            if (done) return;
            p.sh.fail();
            p.hs.fail();
        }
    };

    // The H side of device t, on the context's second lane (own stream and scratch) BESIDE the witness MSMs: uploads, the chain(s)
    // this device owns, the hop of b / c to device 0.  Sliced: every device uploads rows [t*cshare, ...) of A, B and C over its own
    // link into a staging buffer and forwards them to the chain owners over xGMI; the owners start when all pieces have landed.
    int h_helper(uint32_t t) {
        G16Pk* pk = pks[t];
        Ctx* ctx = pk->ctx;
        Release rel{*this};
        std::lock_guard<std::mutex> l1(ctx->lane_mu[1]);
        hipStream_t st = ctx->work_stream();
        if (sliced) {
            const uint64_t lo = std::min<uint64_t>((uint64_t)t * cshare, n_constraints), hi = std::min<uint64_t>(lo + cshare, n_constraints);
            void* stage = nullptr;
            GA_CHECK(ctx->scratch_get("h_stage", 3 * cshare * 32 + 32, &stage));
            for (int k = 0; k < 3; k++) {
                char* mine = (char*)stage + (uint64_t)k * cshare * 32;
                if (hi > lo) {
                    GA_HIP_CHECK(hipMemcpyAsync(mine, (const char*)src[k] + lo * 32, (hi - lo) * 32, hipMemcpyHostToDevice, st));
                    GA_HIP_CHECK(hipMemcpyPeerAsync((char*)chain_buf[k] + lo * 32, pks[owner[k]]->ctx->device, mine, ctx->device, (hi - lo) * 32, st));
                }
                if (owner[k] == t) GA_CHECK(h_pad(pk, chain_buf[k], n_constraints, st));
            }
            GA_HIP_CHECK(hipStreamSynchronize(st));
            if (!hs.barrier(0)) return GA_OK;   // every device's rows have landed on the chain owners
        } else {
            for (int k = 0; k < 3; k++)
                if (owner[k] == t) GA_CHECK(h_upload(pk, src[k], n_constraints, chain_buf[k], st));
        }
        for (int k = 0; k < 3; k++)
            if (owner[k] == t) {
                GA_CHECK(ntt_domain_h_chain<C>(pk->dom, chain_buf[k]));
                if (t != 0) GA_HIP_CHECK(hipMemcpyPeerAsync(dev0_buf[k], pks[0]->ctx->device, chain_buf[k], ctx->device, pk->n * 32, st));
            }
        GA_HIP_CHECK(hipStreamSynchronize(st));
        rel.done = true;
        return GA_OK;
    }

    // device 0, once every chain has arrived: h, then every device gets its slice of h[:n-1]
    int finish_h() {
        G16Pk* pk = pks[0];
        Ctx* ctx = pk->ctx;
        GA_CHECK(ntt_domain_h_combine<C>(pk->dom, dev0_buf[0], dev0_buf[1], dev0_buf[2]));
        for (uint32_t q = 1; q < n; q++) {
            const G16Vec& z = pks[q]->vec[GA_KEY_G1_Z];
            if (z.len) GA_HIP_CHECK(hipMemcpyPeerAsync(h_slice[q], pks[q]->ctx->device, (const char*)dev0_buf[0] + z.off * 32, ctx->device, z.len * 32, ctx->stream));
        }
        GA_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        h_slice[0] = (char*)dev0_buf[0] + pk->vec[GA_KEY_G1_Z].off * 32;
        return GA_OK;
    }

    int worker(uint32_t t) {
        G16Pk* pk = pks[t];
        Ctx* ctx = pk->ctx;
        SlotLease slot(ctx);
        std::lock_guard<std::mutex> g(ctx->mu);   // one proof at a time per device (icicle.go:821-823)
        HelperThread helper;                      // (declared before `rel`: the barriers are released before the helper is joined)
        Release rel{*this};
        ctx->tun.read_env();
        // buffers first, so that peers can address them after barrier 0
        for (int k = 0; k < 3; k++) {
            if (owner[k] == t) GA_CHECK(h_buffer(pk, slot, k, &chain_buf[k]));
            if (t == 0) GA_CHECK(h_buffer(pk, slot, k, &dev0_buf[k]));
        }
        // a base-range shard receives its slice of h, a window shard all of it
        if (t != 0 && pk->vec[GA_KEY_G1_Z].len) GA_CHECK(ctx->scratch_get("h_slice", pk->vec[GA_KEY_G1_Z].len * 32, &h_slice[t]));
        if (!sh.barrier(0)) return GA_OK;
        GA_CHECK(witness_upload(pk, slot, w, nb_public));
        helper.start(ctx, 1, [this, t] { return h_helper(t); });   // (every device has a part: it owns a chain, or the upload is sliced)
        WitnessShared wsh;
        bool did_k = false;
        GA_HIP_CHECK(hipEventCreateWithFlags(&wsh.w_ev, hipEventDisableTiming));
        GA_CHECK(witness_msms<C>(pk, slot, nb_public, wsh, &parts[t], &did_k));
        GA_CHECK(helper.join());
        if (!sh.barrier(1)) return GA_OK;
        if (t == 0) GA_CHECK(finish_h());
        if (!sh.barrier(2)) return GA_OK;
        XYZZ<F1> z;
        GA_CHECK(z_msm<C>(pk, h_slice[t], &z));
        parts[t].krs = add(parts[t].krs, z);
        sh.barrier(3);
        rel.done = true;
        return GA_OK;
    }
};

template <class C>
static int prove_multi(G16Pk* const* pks, uint32_t n, const void* w, const void* a, const void* b, const void* c, uint64_t n_constraints,
                       uint64_t nb_public, const void* r, const void* s, void* proof_out) {
    MultiProof<C> p{pks, n, w, {a, b, c}, n_constraints, nb_public};
    {
        std::vector<HelperThread> workers(n);
        typename MultiProof<C>::Release rel{p};   // (a worker thread that cannot be started: the ones already waiting are released, then joined)
        for (uint32_t t = 1; t < n; t++) workers[t].start(pks[t]->ctx, 0, [&p, t] { return p.worker(t); });
        workers[0].run_here(pks[0]->ctx, 0, [&p] { return p.worker(0); });
        rel.done = true;
        int rc = GA_OK;
        for (uint32_t t = n; t-- > 0;) {   // the failure reported, code and text, is the one of the first device that has one
            const int rc_t = workers[t].join();
            if (rc_t != GA_OK) rc = rc_t;
        }
        GA_CHECK(rc);
    }
    G16Partials<C> sum;
    for (const G16Partials<C>& q : p.parts) {
        sum.ar = add(sum.ar, q.ar);
        sum.bs1 = add(sum.bs1, q.bs1);
        sum.krs = add(sum.krs, q.krs);
        sum.bs2 = add(sum.bs2, q.bs2);
    }
    return finish<C>(pks[0], sum, r, s, proof_out);
}

// ---- the drivers of the proving entry points (g16.hip.h; the entry points are g16_abi.hip) -------------------------------------------
// ga_g16_prove, and the proof inside ga_g16_prove_oneshot and ga_g16_prove_multi with one key
int g16_prove_run(G16Pk* pk, const void* w, const void* a, const void* b, const void* c, uint64_t n_constraints, uint64_t nb_public,
                  const void* r, const void* s, void* proof_out) {
    GA_PK_USE(pk);
    GA_CHECK(check_unsharded(pk));
    // Two callers may be inside at once (two goroutines proving on one device).  The first holds the device lock and works on
    // lanes 0/1 (witness MSMs / H side, prove_partial).  The second finds the device busy and computes its proof on lanes 2/3 --
    // own streams, own scratch namespaces -- so the two proofs run CONCURRENTLY: uploads hide behind the other proof's kernels
    // and the kernels interleave.  When lane 2 is taken as well, or while the profiler records stages, or with GA_G16_LANES=1,
    // the caller stages its solution in its input slot and queues for the device.  The host epilogue always runs outside the
    // device lock.  ga_g16_lane_stats reports how the calls of a context were scheduled.
    // A lane-2 proof that cannot get its scratch (precompute = 0 fills HBM with tables beside ONE caller's scratch: at 2^26 a second
    // caller's 77 GiB are not there) gives back what lanes 2/3 hold and queues for the device like a third caller would -- a proof
    // is slower then, never failed.
    Ctx* ctx = pk->ctx;
    SlotLease slot(ctx);
    std::unique_lock<std::mutex> dev(ctx->mu, std::try_to_lock);
    std::unique_lock<std::mutex> lane2(ctx->lane_mu[2], std::defer_lock);
    hipSetDevice(ctx->device);
    for (int attempt = 0;; attempt++) {
        bool preloaded = false;
        int lane = 0;
        if (!dev.owns_lock()) {
            if (attempt == 0 && !ctx->profiling && ctx->tun.g16_lanes > 1 && lane2.try_lock()) {
                lane = 2;
                ctx->stat_lane2++;
            } else {
                GA_CHECK(preload_solution(pk, slot, w, a, b, c, n_constraints, nb_public));
                preloaded = true;
                dev.lock();
                ctx->stat_queued++;
            }
        }
        if (lane == 0 && !preloaded) ctx->stat_lane0++;
        int partial_rc = GA_OK;
        {
            LaneScope on_lane(lane);
            if (lane == 0) ctx->tun.read_env();
            const int rc = GA_DISPATCH(Scope::FULL, pk->curve, GA_NO_GROUP, {
                G16Partials<C> part;
                partial_rc = prove_partial<C>(pk, slot, preloaded, w, a, b, c, n_constraints, nb_public, &part);
                if (partial_rc == GA_OK) {
                    const bool profiling = ctx->profiling;
                    if (lane == 0 && !profiling) dev.unlock();   // the stage list of the profiler is guarded by the device lock
                    if (lane == 2) lane2.unlock();
                    return finish<C>(pk, part, r, s, proof_out);
                }
            });
            if (partial_rc == GA_OK) return rc;   // the proof is finished (or the dispatch refused the key's curve)
        }
        if (partial_rc != GA_ERR_NOMEM || lane != 2) return partial_rc;
        // (everything prove_partial started on lanes 2/3 has joined; hipFree synchronises with what their streams still hold)
        ctx->scratch_free_lanes(2);
        ctx->stat_lane2--;
        lane2.unlock();
    }
}

// out[0..3] = ga_g16_prove calls of this context that ran on lanes 0/1, on lanes 2/3 beside another proof, that staged their
// inputs and queued for the device, and proofs whose H side ran on a partner lane (any entry point); out[4..5] = device bytes
// of scratch held by lanes 0/1 and by lanes 2/3
int g16_lane_stats(Ctx* ctx, uint64_t* out6) {
    const uint64_t stats[6] = {ctx->stat_lane0, ctx->stat_lane2, ctx->stat_queued, ctx->stat_split, 0, 0};
    memcpy(out6, stats, sizeof stats);
    std::lock_guard<std::mutex> g(ctx->scratch_mu);
    for (const auto& kv : ctx->scratch) out6[kv.second.lane < 2 ? 4 : 5] += kv.second.bytes;
    return GA_OK;
}

// `count` proofs under one key: a loop of groth16.Prove over one ProvingKey (prove.go:130-315; the reference has no batch entry
// point) as one caller of the device -- prove_batch on lane 0 under the device lock, then the epilogues outside it (finish_batch).  A
// ga_g16_prove arriving meanwhile finds the device busy and proves on lanes 2/3 as beside any other proof.
int g16_prove_batch_run(G16Pk* pk, uint32_t count, const void* const* w, const void* const* a, const void* const* b, const void* const* c,
                        uint64_t n_constraints, uint64_t nb_public, const void* r, const void* s, void* proofs_out) {
    for (uint32_t j = 0; j < count; j++)
        if (!w[j] || !a[j] || !b[j] || !c[j]) {
            set_error("%s: null pointer in solution %u (%s[%u])", current_entry(), j, !w[j] ? "w" : !a[j] ? "a" : !b[j] ? "b" : "c", j);
            return GA_ERR_INVALID;
        }
    GA_PK_USE(pk);
    GA_CHECK(check_unsharded(pk));
    GA_CHECK(check_nb_constraints(pk, n_constraints));
    GA_CHECK(check_nb_public(pk, nb_public));
    Ctx* ctx = pk->ctx;
    return GA_DISPATCH(Scope::FULL, pk->curve, GA_NO_GROUP, {
        std::vector<G16Partials<C>> parts(count);
        {
            std::unique_lock<std::mutex> dev(ctx->mu);
            hipSetDevice(ctx->device);
            ctx->tun.read_env();
            GA_CHECK(prove_batch<C>(pk, count, w, a, b, c, n_constraints, nb_public, parts.data()));
            // (the stage list of the profiler is guarded by the device lock)
            if (ctx->profiling) return finish_batch<C>(pk, parts, r, s, proofs_out, /*serial=*/true);
        }
        return finish_batch<C>(pk, parts, r, s, proofs_out, /*serial=*/false);
    });
}

// One proof on a key that is NOT kept on the device (the Go package's default, PinToGPU = false, as icicle.go:797-805): the key
// goes up as plain vectors WHILE the proof runs -- the uploader thread of pk_create_from_struct copies A, B, K, G2.B, Z in the order
// the MSMs consume them, every MSM waits for its own vector only -- and is dropped afterwards.  Same proof bytes as
// ga_g16_pk_create(precompute = -1) + ga_g16_prove + ga_g16_pk_destroy, in about the time of the longer of the two (PCIe, device)
// instead of their sum.  No host pointer is used after the call returns (the uploader is joined before the key is freed).
int g16_prove_oneshot_run(Ctx* ctx, const ga_g16_key* key, const void* w, const void* a, const void* b, const void* c, uint64_t n_constraints,
                          uint64_t nb_public, const void* r, const void* s, void* proof_out) {
    trace_event("ga_g16_prove_oneshot", 0);
    struct InFlight {   // pageable uploads of this context take turns while the key is on its way (common.hip.h)
        Ctx* c;
        explicit InFlight(Ctx* x) : c(x) { c->oneshot_inflight++; }
        ~InFlight() { c->oneshot_inflight--; }
    } inflight(ctx);
    G16Pk* pk = nullptr;
    GA_CHECK(pk_create_run(ctx, key, &pk, /*defer_uploads=*/true));
    struct Drop {   // whatever happens below, the uploader is joined and the key freed before the host vectors go out of scope
        G16Pk* pk;
        ~Drop() {
            pk_destroy(pk);
            trace_event("key dropped", 0);
        }
    } drop{pk};
    trace_event("key reserved, uploader started", 0);
    const int rc = g16_prove_run(pk, w, a, b, c, n_constraints, nb_public, r, s, proof_out);
    trace_event("proof done", rc);
    return rc;
}

int g16_prove_partial_run(G16Pk* pk, const void* w, const void* a, const void* b, const void* c, uint64_t n_constraints, uint64_t nb_public, void* partials_out) {
    GA_PK_USE(pk);
    SlotLease slot(pk->ctx);   // always slot first, device lock second (g16_prove_run's order)
    CtxLock g(pk->ctx);
    return GA_DISPATCH(Scope::FULL, pk->curve, GA_NO_GROUP, {
        G16Partials<C> part;
        GA_CHECK(prove_partial<C>(pk, slot, false, w, a, b, c, n_constraints, nb_public, &part));
        part.store(partials_out);
    });
}

int g16_finish_run(G16Pk* pk, const void* partials_sum, const void* r, const void* s, void* proof_out) {
    GA_PK_USE(pk);
    return GA_DISPATCH(Scope::FULL, pk->curve, GA_NO_GROUP, {
        G16Partials<C> sum;
        sum.load(partials_sum);
        return finish<C>(pk, sum, r, s, proof_out);
    });
}

// ---- pieces of a sharded proof (multi-GPU orchestration by the caller: gnark_amd/multigpu.py over RCCL, or g16_prove_multi_run) ----
int g16_witness_partial_run(G16Pk* pk, const void* w, uint64_t nb_public, void* partials_out) {
    GA_PK_USE(pk);
    SlotLease slot(pk->ctx);
    CtxLock g(pk->ctx);
    return GA_DISPATCH(Scope::FULL, pk->curve, GA_NO_GROUP, {
        G16Partials<C> part;
        GA_CHECK(witness_upload(pk, slot, w, nb_public));
        WitnessShared sh;
        GA_HIP_CHECK(hipEventCreateWithFlags(&sh.w_ev, hipEventDisableTiming));
        bool did_k = false;
        GA_CHECK(witness_msms<C>(pk, slot, nb_public, sh, &part, &did_k));
        part.store(partials_out);
    });
}

int g16_h_chain_run(G16Pk* pk, const void* host_v, void* dev_buf, uint64_t n_constraints) {
    GA_PK_USE(pk);
    GA_CHECK(check_nb_constraints(pk, n_constraints));
    LaneLock g(pk->ctx);   // beside the witness MSMs of the same shard when the caller runs them from another thread
    hipStream_t st = pk->ctx->work_stream();
    GA_CHECK(host_v ? h_upload(pk, host_v, n_constraints, dev_buf, st) : h_pad(pk, dev_buf, n_constraints, st));
    GA_CHECK(GA_DISPATCH(Scope::FULL, pk->curve, GA_NO_GROUP, return ntt_domain_h_chain<C>(pk->dom, dev_buf)));
    GA_HIP_CHECK(hipStreamSynchronize(st));   // the buffer is handed to another stream / device next
    return GA_OK;
}

int g16_h_combine_run(G16Pk* pk, void* a_dev, const void* b_dev, const void* c_dev) {
    GA_PK_USE(pk);
    LaneLock g(pk->ctx);
    GA_CHECK(GA_DISPATCH(Scope::FULL, pk->curve, GA_NO_GROUP, return ntt_domain_h_combine<C>(pk->dom, a_dev, b_dev, c_dev)));
    GA_HIP_CHECK(hipStreamSynchronize(pk->ctx->work_stream()));
    return GA_OK;
}

int g16_z_partial_run(G16Pk* pk, const void* h_slice_dev, void* partial_out) {
    if (abi_null_argument(!h_slice_dev && pk->vec[GA_KEY_G1_Z].len)) return GA_ERR_INVALID;
    GA_PK_USE(pk);
    CtxLock g(pk->ctx);
    return GA_DISPATCH(Scope::FULL, pk->curve, GA_NO_GROUP, {
        typedef Fe<typename C::FpP> F1;
        XYZZ<F1> z;
        GA_CHECK(z_msm<C>(pk, h_slice_dev, &z));
        host_store_jac<F1>(partial_out, z);
    });
}

int g16_prove_multi_run(G16Pk* const* pks, uint32_t n, const void* w, const void* a, const void* b, const void* c, uint64_t n_constraints,
                        uint64_t nb_public, const void* r, const void* s, void* proof_out) {
    for (uint32_t t = 0; t < n; t++) {
        const bool by_range = pks[t] && pks[t]->shard_count == n && pks[t]->shard_index == t && pks[t]->win_count == 1;
        const bool by_window = pks[t] && pks[t]->win_count == n && pks[t]->win_index == t && pks[t]->shard_count == 1;
        if (!pks[t] || pks[t]->curve != pks[0]->curve || pks[t]->n != pks[0]->n || pks[t]->nb_wires != pks[0]->nb_wires ||
            !(n == 1 || by_range || by_window) || (pks[t]->win_count > 1) != (pks[0]->win_count > 1)) {
            set_error("%s: keys[%u] must be shard %u of %u of the same proving key (all by base range or all by windows)", current_entry(), t, t, n);
            return GA_ERR_INVALID;
        }
        for (uint32_t q = 0; q < t; q++)
            if (pks[q]->ctx == pks[t]->ctx) {
                set_error("%s: keys[%u] and keys[%u] share a context; one context per shard", current_entry(), q, t);
                return GA_ERR_INVALID;
            }
    }
    if (n == 1) return g16_prove_run(pks[0], w, a, b, c, n_constraints, nb_public, r, s, proof_out);
    std::vector<std::unique_ptr<PkUse>> uses;
    for (uint32_t t = 0; t < n; t++) {
        uses.emplace_back(new PkUse(pks[t]));
        if (!uses.back()->ok) {
            set_error("%s: keys[%u] is being destroyed", current_entry(), t);
            return GA_ERR_STATE;
        }
    }
    // the solution's sizes against the key, before any thread starts or anything is launched
    GA_CHECK(check_nb_constraints(pks[0], n_constraints));
    for (uint32_t t = 0; t < n; t++) GA_CHECK(check_nb_public(pks[t], nb_public));
    // One multi-device proof at a time per process: every worker thread holds its device's lock while it waits for the others at
    // the barriers, so two calls over the same devices could each hold one lock the other needs (A holds dev0 and waits for its
    // worker on dev1, B holds dev1 and waits for its worker on dev0).  A sharded proof occupies all its devices anyway.
    static std::mutex multi_mu;
    std::lock_guard<std::mutex> multi_guard(multi_mu);
    for (uint32_t t = 0; t < n; t++)   // peer access both ways between device 0 and the others (errors = already enabled / same device)
        for (uint32_t q = 0; q < n; q++)
            if (q != t && (t == 0 || q == 0) && pks[t]->ctx->device != pks[q]->ctx->device) {
                hipSetDevice(pks[t]->ctx->device);
                (void)hipDeviceEnablePeerAccess(pks[q]->ctx->device, 0);
                (void)hipGetLastError();
            }
    return GA_DISPATCH(Scope::FULL, pks[0]->curve, GA_NO_GROUP, return (prove_multi<C>(pks, n, w, a, b, c, n_constraints, nb_public, r, s, proof_out)));
}

int g16_commit_run(G16Pk* pk, uint32_t index, const void* values, uint64_t n_values, void* commitment_out, void* pok_out) {
    GA_PK_USE(pk);
    CtxLock g(pk->ctx);
    return GA_DISPATCH(Scope::FULL, pk->curve, GA_NO_GROUP, return commit<C>(pk, index, values, n_values, commitment_out, pok_out));
}

int g16_fold_pok_run(int curve, const void* poks, uint64_t n, const void* challenge, void* out) {
    return GA_DISPATCH(Scope::FULL, curve, GA_NO_GROUP, return fold_pok<C>(poks, n, challenge, out));
}

}  // namespace ga

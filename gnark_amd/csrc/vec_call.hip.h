// The driver kit of the point and Fr vector calls (fixed_base, ec_ntt, scale_points, check_points, sparse_sums, fr_sparse / fr_setup):
// what the host side of every one of them does around its own kernels.  Host code only; a piece lives here when at least two drivers
// use it.  A driver takes its whole scratch first (an allocation failure leaves nothing in flight), then declares a StreamDrain, then
// walks its input in chunks of clamp_chunk() elements: chunk_in, its kernels on capped_grid() blocks with a RedoList between the fast
// kernel and the exact one, launch_to_affine (fixed_base.hip.h, beside its kernel), chunk_out -- and synchronises once at the end.
#pragma once
#include "common.hip.h"

namespace ga {

constexpr uint64_t VEC_MAX_CHUNK = 1ull << 30;   // elements per pass at the most: indices inside a pass are 32-bit

// every return, an error's included, leaves with the stream idle: the copies in flight, the caller's buffers and the host-side plan
// outlive the work that reads them
struct StreamDrain {
    hipStream_t st;
    ~StreamDrain() { hipStreamSynchronize(st); }
};

// A whole operand brought to the device when it is a host pointer, for the calls that do not walk their input in chunks (the MSMs,
// the table MSMs, ga_fr_poly_evaluate, ga_fr_vec_mul): its own allocation, released at scope exit, and complete when stage() returns.
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

// elements per pass: the knob (0 = the call's default), at most VEC_MAX_CHUNK, at most n
inline uint64_t clamp_chunk(uint64_t forced, uint64_t dflt, uint64_t n) {
    uint64_t chunk = forced ? forced : dflt;
    if (chunk > VEC_MAX_CHUNK) chunk = VEC_MAX_CHUNK;
    return chunk > n ? n : chunk;
}

// workgroups of `threads` lanes that cover n elements, at most max_blocks (the kernel is grid-stride beyond)
inline unsigned capped_grid(uint64_t n, unsigned threads, unsigned max_blocks) {
    const uint64_t all = (n + threads - 1) / threads;
    return (unsigned)(all < max_blocks ? all : max_blocks);
}

// The lanes a fast kernel flags for the exact kernel behind it, carved from ONE scratch buffer of (entries + header) words: `header`
// words of counters first (a multiple of 4, so the list stays 16-byte aligned; what they hold is the driver's), then the list.
struct RedoList {
    uint32_t* words = nullptr;   // the header
    uint32_t* list = nullptr;
    int get(Ctx* ctx, const char* key, uint64_t entries, unsigned header) {
        GA_CHECK(ctx->scratch_get(key, (entries + header) * 4, (void**)&words));
        list = words + header;
        return GA_OK;
    }
};

// cn elements of an operand from element `done` on: read where they are on the device, else copied (async) into `staging`
template <class T>
int chunk_in(hipStream_t st, bool on_device, const T* p, uint64_t done, uint64_t cn, T* staging, const T** src) {
    *src = on_device ? p + done : staging;
    if (!on_device && cn) GA_HIP_CHECK(hipMemcpyAsync(staging, p + done, cn * sizeof(T), hipMemcpyHostToDevice, st));
    return GA_OK;
}
// its mirror: a result the kernels left in `staging` goes to the host (async); one written in place on the device is there already
template <class T>
int chunk_out(hipStream_t st, bool on_device, T* p, uint64_t done, uint64_t cn, const T* staging) {
    if (!on_device) GA_HIP_CHECK(hipMemcpyAsync(p + done, staging, cn * sizeof(T), hipMemcpyDeviceToHost, st));
    return GA_OK;
}

}  // namespace ga

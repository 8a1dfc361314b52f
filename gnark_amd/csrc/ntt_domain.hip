// Non-templated accessors of the fft.Domain analogue (see ntt.hip.h), and the drivers of ga_fft[_batch] and ga_compute_h[_batch].
#include "plonk.hip.h"
#include "plonk_verify.hip.h"
#include "vec_call.hip.h"
namespace ga {
void plonk_fixed_delete(PlonkFixed* fx) { plonk_fixed_destroy(fx); }
Domain* plonk_fixed_domain0(PlonkFixed* fx) { return fx->d0; }
void plonk_vk_delete(PlonkVk* vk) { plonk_vk_free(vk); }
Domain* plonk_vk_domain0(PlonkVk* vk) { return vk->d0; }
void ntt_domain_delete(Domain* d) {
    if (!d) return;
    domain_free(d);
    delete d;
}
Domain* ntt_domain_take_spare(Ctx* ctx, int curve, uint64_t n) {
    std::lock_guard<std::mutex> g(ctx->spare_mu);
    Domain* d = ctx->spare_domain;
    if (!d || d->curve != curve || d->n != n) return nullptr;
    ctx->spare_domain = nullptr;
    return d;
}
void ntt_domain_give_spare(Ctx* ctx, Domain* d) {
    if (!d) return;
    const char* e = getenv("GA_DOMAIN_SPARE");
    Domain* old = nullptr;
    if (e && atoi(e) == 0) {
        old = d;
    } else {
        std::lock_guard<std::mutex> g(ctx->spare_mu);
        old = ctx->spare_domain;
        ctx->spare_domain = d;
    }
    ntt_domain_delete(old);
}
int ntt_domain_curve(const Domain* d) { return d->curve; }
uint64_t ntt_domain_size(const Domain* d) { return d->n; }
Ctx* ntt_domain_ctx(const Domain* d) { return d->ctx; }

// `count` transforms of one size in ONE launch chain (the vector is the grid's y dimension of every pass, ntt.hip.h)
int ntt_domain_fft_run(Domain* d, void* data, uint32_t count, int direction, int decimation, int on_coset, bool on_device) {
    Ctx* c = d->ctx;
    const size_t bytes = (size_t)count * d->n * 32;
    void* dev = data;
    if (!on_device) GA_CHECK(c->scratch_get("fft_io", bytes, &dev));
    StreamDrain drain{c->stream};
    if (!on_device) GA_HIP_CHECK(hipMemcpyAsync(dev, data, bytes, hipMemcpyHostToDevice, c->stream));
    GA_CHECK(GA_DISPATCH(Scope::G1_FR, d->curve, GA_NO_GROUP, return ntt_domain_fft<C>(d, dev, direction, decimation, on_coset, count)));
    if (!on_device) GA_HIP_CHECK(hipMemcpyAsync(data, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    GA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GA_OK;
}

// computeH for `count` solutions of one circuit (a loop of prove.go:346-389 over the solutions): rows of n_constraints elements go into
// rows of the cardinality, zero-padded; every transform is one batched launch chain and the point-wise step one launch
int ntt_domain_compute_h_run(Domain* d, const void* a, const void* b, const void* cc, uint32_t count, uint64_t n_constraints, void* h_out,
                             bool on_device) {
    Ctx* c = d->ctx;
    const size_t full = d->n * 32, part = n_constraints * 32;
    void* dst[3];
    GA_CHECK(c->scratch_get("compute_h_a", (size_t)count * full, &dst[0]));
    GA_CHECK(c->scratch_get("compute_h_b", (size_t)count * full, &dst[1]));
    GA_CHECK(c->scratch_get("compute_h_c", (size_t)count * full, &dst[2]));
    StreamDrain drain{c->stream};
    const void* src[3] = {a, b, cc};
    const hipMemcpyKind in = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    for (int k = 0; k < 3; k++) {
        if (part == full) {
            GA_HIP_CHECK(hipMemcpyAsync(dst[k], src[k], (size_t)count * full, in, c->stream));
        } else if (part) {   // (rows of n_constraints elements into rows of n)
            for (uint32_t j = 0; j < count; j++)
                GA_HIP_CHECK(hipMemcpyAsync((char*)dst[k] + j * full, (const char*)src[k] + j * part, part, in, c->stream));
        }
        GA_CHECK(GA_DISPATCH(Scope::G1_FR, d->curve, GA_NO_GROUP, return util_pad_fr_batch<C>(c, dst[k], n_constraints, d->n, count, c->stream)));
    }
    GA_CHECK(GA_DISPATCH(Scope::G1_FR, d->curve, GA_NO_GROUP, return ntt_domain_compute_h<C>(d, dst[0], dst[1], dst[2], count)));
    GA_HIP_CHECK(hipMemcpyAsync(h_out, dst[0], (size_t)count * full, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    GA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GA_OK;
}
}  // namespace ga

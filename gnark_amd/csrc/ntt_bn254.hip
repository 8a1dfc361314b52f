// Explicit instantiation: Fr NTT / computeH, bn254 (see ntt.hip.h).
#include "ntt.hip.h"
namespace ga {
template <>
int ntt_domain_new<Bn254>(Ctx* ctx, uint64_t n, Domain** out) {
    Domain* d = new Domain();
    int rc = domain_init<Bn254::FrP>(ctx, d, Bn254::ID, n);
    if (rc != GA_OK) {
        domain_free(d);
        delete d;
        return rc;
    }
    *out = d;
    return GA_OK;
}
template <>
int ntt_domain_fft<Bn254>(Domain* d, void* d_data, int direction, int decimation, int on_coset, uint64_t batch) {
    return ntt_fft<Bn254::FrP>(d, (uint32_t*)d_data, direction, decimation, on_coset, batch);
}
template <>
int ntt_domain_h_chain<Bn254>(Domain* d, void* d_v, uint64_t batch) {
    return ntt_compute_h_chain<Bn254::FrP>(d, (uint32_t*)d_v, batch);
}
template <>
int ntt_domain_h_combine<Bn254>(Domain* d, void* d_a, const void* d_b, const void* d_c, uint64_t batch) {
    return ntt_compute_h_combine<Bn254::FrP>(d, (uint32_t*)d_a, (const uint32_t*)d_b, (const uint32_t*)d_c, batch);
}
template <>
int ntt_domain_compute_h<Bn254>(Domain* d, void* d_a, void* d_b, void* d_c, uint64_t batch) {
    return ntt_compute_h<Bn254::FrP>(d, (uint32_t*)d_a, (uint32_t*)d_b, (uint32_t*)d_c, batch);
}
}  // namespace ga

// Explicit instantiation: Fr NTT / computeH, bls12377 (see ntt.hip.h).
#include "ntt.hip.h"
namespace ga {
template <>
int ntt_domain_new<Bls12377>(Ctx* ctx, uint64_t n, Domain** out) {
    Domain* d = new Domain();
    int rc = domain_init<Bls12377::FrP>(ctx, d, Bls12377::ID, n);
    if (rc != GA_OK) {
        domain_free(d);
        delete d;
        return rc;
    }
    *out = d;
    return GA_OK;
}
template <>
int ntt_domain_fft<Bls12377>(Domain* d, void* d_data, int direction, int decimation, int on_coset, uint64_t batch) {
    return ntt_fft<Bls12377::FrP>(d, (uint32_t*)d_data, direction, decimation, on_coset, batch);
}
template <>
int ntt_domain_h_chain<Bls12377>(Domain* d, void* d_v, uint64_t batch) {
    return ntt_compute_h_chain<Bls12377::FrP>(d, (uint32_t*)d_v, batch);
}
template <>
int ntt_domain_h_combine<Bls12377>(Domain* d, void* d_a, const void* d_b, const void* d_c, uint64_t batch) {
    return ntt_compute_h_combine<Bls12377::FrP>(d, (uint32_t*)d_a, (const uint32_t*)d_b, (const uint32_t*)d_c, batch);
}
template <>
int ntt_domain_compute_h<Bls12377>(Domain* d, void* d_a, void* d_b, void* d_c, uint64_t batch) {
    return ntt_compute_h<Bls12377::FrP>(d, (uint32_t*)d_a, (uint32_t*)d_b, (uint32_t*)d_c, batch);
}
}  // namespace ga

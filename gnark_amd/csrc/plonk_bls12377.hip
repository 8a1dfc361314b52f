// Explicit instantiation: PLONK quotient / grand product / batch inversion, bls12377 (see plonk.hip.h, plonk_batch.hip.h).
#include "plonk_batch.hip.h"
namespace ga {
template <>
int plonk_domain_quotient<Bls12377>(Domain* d0, Domain* d1, const PlonkQuotientArgs& args, void* h_out) {
    return plonk_quotient<Bls12377::FrP>(d0, d1, args, h_out);
}
template <>
int plonk_domain_fixed_create<Bls12377>(Domain* d0, Domain* d1, const PlonkQuotientArgs& args, PlonkFixed** out) {
    return plonk_fixed_create<Bls12377::FrP>(d0, d1, args, out);
}
template <>
int fr_vec_batch_inverse<Bls12377>(Ctx* ctx, void* v, uint64_t n, bool on_device) {
    return fr_batch_inverse<Bls12377::FrP>(ctx, v, n, on_device);
}
template <>
int fr_vec_lincomb<Bls12377>(Ctx* ctx, uint64_t n, int k, const void* const* vecs, const void* scalars, void* out, bool on_device) {
    return fr_lincomb<Bls12377::FrP>(ctx, n, k, vecs, scalars, out, on_device);
}
template <>
int plonk_domain_build_z_batch<Bls12377>(Domain* d0, const void* L, const void* R, const void* O, const int64_t* perm, const void* betas,
                                       const void* gammas, uint32_t count, PlonkBatchKnobs knobs, bool on_device, void* z_out) {
    return plonk_build_z<Bls12377::FrP>(d0, L, R, O, perm, betas, gammas, count, knobs, on_device, z_out);
}
template <>
int plonk_domain_quotient_pinned_batch<Bls12377>(PlonkFixed* fx, const PlonkQuotientArgs* args, uint32_t count, PlonkBatchKnobs knobs, void* h_out) {
    return plonk_quotient_pinned<Bls12377::FrP>(fx, args, count, knobs, h_out);
}
template <>
int kzg_domain_divide_batch<Bls12377>(Ctx* ctx, const void* const* d_polys, uint64_t n, uint32_t count, const void* points, void* d_quot,
                                    uint64_t quot_stride, void* d_values, uint64_t scan_threads, std::vector<uint32_t>* stage) {
    return kzg_divide_by_linear<Bls12377::FrP>(ctx, d_polys, n, count, points, (uint32_t*)d_quot, quot_stride, (uint32_t*)d_values, scan_threads, *stage);
}
}  // namespace ga

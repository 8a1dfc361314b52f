// Explicit instantiation: synthetic-input / checking kernels, bls12377 (see util.hip.h).
#include "util.hip.h"
namespace ga {
template int util_gen_bases<Bls12377, GA_G1>(Ctx*, uint64_t, size_t, void*, void*, uint64_t);
template int util_gen_scalars<Bls12377>(Ctx*, uint64_t, size_t, void*);
template int util_fr_dot<Bls12377>(Ctx*, const void*, const void*, size_t, void*);
template int util_fr_vec_mul<Bls12377>(Ctx*, const void*, const void*, size_t, void*);
template int util_gather_fr<Bls12377>(Ctx*, void*, const void*, const uint32_t*, size_t);
template int util_gather_fr_batch<Bls12377>(Ctx*, void*, const void*, const uint32_t*, size_t, uint32_t, uint64_t, uint64_t);
template int util_pad_fr_batch<Bls12377>(Ctx*, void*, uint64_t, uint64_t, uint32_t, hipStream_t);
template int msm_plan<Bls12377>(int, size_t, int*, int*);
template int msm_plan_table<Bls12377>(size_t, int*, int*, bool);
}  // namespace ga

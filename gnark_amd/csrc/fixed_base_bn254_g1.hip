// Explicit instantiation: fixed-base batch scalar multiplication, bn254 G1 (see fixed_base.hip.h).
#include "fixed_base.hip.h"
namespace ga {
template int fixed_base_run<Bn254, GA_G1>(Ctx*, const void*, const void*, size_t, unsigned, void*, int, uint64_t);
template int fixed_base_plan_abi<Bn254>(size_t, int, int*, int*);
}  // namespace ga

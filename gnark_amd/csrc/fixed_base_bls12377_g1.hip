// Explicit instantiation: fixed-base batch scalar multiplication, bls12377 G1 (see fixed_base.hip.h).
#include "fixed_base.hip.h"
namespace ga {
template int fixed_base_run<Bls12377, GA_G1>(Ctx*, const void*, const void*, size_t, unsigned, void*, int, uint64_t);
template int fixed_base_plan_abi<Bls12377>(size_t, int, int*, int*);
}  // namespace ga

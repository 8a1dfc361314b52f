// Explicit instantiation: fixed-base batch scalar multiplication, bls12381 G1 (see fixed_base.hip.h).
#include "fixed_base.hip.h"
namespace ga {
GA_INSTANTIATE_FIXED_BASE(Bls12381, GA_G1)
GA_INSTANTIATE_FIXED_BASE_PLAN(Bls12381)
}  // namespace ga

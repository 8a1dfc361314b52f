// Explicit instantiation: fixed-base batch scalar multiplication, bn254 G1 (see fixed_base.hip.h).
#include "fixed_base.hip.h"
namespace ga {
GA_INSTANTIATE_FIXED_BASE(Bn254, GA_G1)
GA_INSTANTIATE_FIXED_BASE_PLAN(Bn254)
}  // namespace ga

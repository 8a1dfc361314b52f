// Explicit instantiation: fixed-base batch scalar multiplication, bls12381 G2 (see fixed_base.hip.h).
#include "fixed_base.hip.h"
namespace ga {
GA_INSTANTIATE_FIXED_BASE(Bls12381, GA_G2)
}  // namespace ga

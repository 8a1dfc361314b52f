// Explicit instantiation: fixed-base batch scalar multiplication, bn254 G2 (see fixed_base.hip.h).
#include "fixed_base.hip.h"
namespace ga {
GA_INSTANTIATE_FIXED_BASE(Bn254, GA_G2)
}  // namespace ga

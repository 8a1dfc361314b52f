// Explicit instantiation: pairing products, bls12381 (see pairing.hip.h).
#include "pairing.hip.h"
namespace ga {
GA_INSTANTIATE_PAIRING(Bls12381)
}  // namespace ga

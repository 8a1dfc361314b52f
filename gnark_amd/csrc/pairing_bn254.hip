// Explicit instantiation: pairing products, bn254 (see pairing.hip.h).
#include "pairing.hip.h"
namespace ga {
GA_INSTANTIATE_PAIRING(Bn254)
}  // namespace ga

// Explicit instantiation: Fr NTT / computeH, bn254 (see ntt.hip.h).
#include "ntt.hip.h"
namespace ga {
GA_INSTANTIATE_NTT(Bn254)
}  // namespace ga

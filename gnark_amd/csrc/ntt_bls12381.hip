// Explicit instantiation: Fr NTT / computeH, bls12381 (see ntt.hip.h).
#include "ntt.hip.h"
namespace ga {
GA_INSTANTIATE_NTT(Bls12381)
}  // namespace ga

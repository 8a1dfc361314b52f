// Explicit instantiation: Fr NTT / computeH, bls12377 (see ntt.hip.h).
#include "ntt.hip.h"
namespace ga {
GA_INSTANTIATE_NTT(Bls12377)
}  // namespace ga

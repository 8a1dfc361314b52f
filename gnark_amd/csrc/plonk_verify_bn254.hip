// Explicit instantiation: the scalar side and the drivers of plonk.Verify, bn254 (see plonk_verify.hip.h).
#include "plonk_verify.hip.h"
namespace ga {
GA_INSTANTIATE_PLONK_VERIFY(Bn254)
}  // namespace ga

// Explicit instantiation: the scalar side and the drivers of plonk.Verify, bls12-381 (see plonk_verify.hip.h).
#include "plonk_verify.hip.h"
namespace ga {
GA_INSTANTIATE_PLONK_VERIFY(Bls12381)
}  // namespace ga

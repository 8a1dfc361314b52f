// Explicit instantiation: Pippenger MSM, bls12381 G2 (see msm.hip.h).
#include "msm.hip.h"
namespace ga {
GA_INSTANTIATE_MSM(Bls12381, GA_G2)
}  // namespace ga

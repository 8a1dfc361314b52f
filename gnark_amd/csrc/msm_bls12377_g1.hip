// Explicit instantiation: Pippenger MSM, bls12377 G1 (see msm.hip.h).
#include "msm.hip.h"
namespace ga {
GA_INSTANTIATE_MSM(Bls12377, GA_G1)
GA_INSTANTIATE_MSM_SCALARS(Bls12377)
}  // namespace ga

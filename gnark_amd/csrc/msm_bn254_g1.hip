// Explicit instantiation: Pippenger MSM, bn254 G1 (see msm.hip.h).
#include "msm.hip.h"
namespace ga {
GA_INSTANTIATE_MSM(Bn254, GA_G1)
GA_INSTANTIATE_MSM_SCALARS(Bn254)
}  // namespace ga

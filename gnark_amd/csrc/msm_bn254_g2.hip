// Explicit instantiation: Pippenger MSM, bn254 G2 (see msm.hip.h).
#include "msm.hip.h"
namespace ga {
GA_INSTANTIATE_MSM(Bn254, GA_G2)
}  // namespace ga

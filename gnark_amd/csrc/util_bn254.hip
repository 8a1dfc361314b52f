// Explicit instantiation: synthetic-input / checking kernels, bn254 (see util.hip.h).
#include "util.hip.h"
namespace ga {
GA_INSTANTIATE_UTIL(Bn254)
GA_INSTANTIATE_UTIL_GROUP(Bn254, GA_G1)
GA_INSTANTIATE_UTIL_GROUP(Bn254, GA_G2)
}  // namespace ga

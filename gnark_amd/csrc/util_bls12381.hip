// Explicit instantiation: synthetic-input / checking kernels, bls12381 (see util.hip.h).
#include "util.hip.h"
namespace ga {
GA_INSTANTIATE_UTIL(Bls12381)
GA_INSTANTIATE_UTIL_GROUP(Bls12381, GA_G1)
GA_INSTANTIATE_UTIL_GROUP(Bls12381, GA_G2)
}  // namespace ga

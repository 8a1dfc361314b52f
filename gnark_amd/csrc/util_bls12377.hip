// Explicit instantiation: synthetic-input / checking kernels, bls12377 (see util.hip.h).
#include "util.hip.h"
namespace ga {
GA_INSTANTIATE_UTIL(Bls12377)
GA_INSTANTIATE_UTIL_GROUP(Bls12377, GA_G1)
}  // namespace ga

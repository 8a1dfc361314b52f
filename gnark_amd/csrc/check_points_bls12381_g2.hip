// Explicit instantiation: batch curve and subgroup checks, bls12381 G2 (see check_points.hip.h).
#include "check_points.hip.h"
namespace ga {
GA_INSTANTIATE_CHECK_POINTS(Bls12381, GA_G2)
}  // namespace ga

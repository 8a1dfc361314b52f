// Explicit instantiation: per-point scalar multiplication, bls12381 G2 (see scale_points.hip.h).
#include "scale_points.hip.h"
namespace ga {
GA_INSTANTIATE_SCALE_POINTS(Bls12381, GA_G2)
}  // namespace ga

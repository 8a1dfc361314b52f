// Explicit instantiation: per-point scalar multiplication, bn254 G1 (see scale_points.hip.h).
#include "scale_points.hip.h"
namespace ga {
GA_INSTANTIATE_SCALE_POINTS(Bn254, GA_G1)
}  // namespace ga

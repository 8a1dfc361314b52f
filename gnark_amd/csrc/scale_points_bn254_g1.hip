// Explicit instantiation: per-point scalar multiplication, bn254 G1 (see scale_points.hip.h).
#include "scale_points.hip.h"
namespace ga {
template int scale_points_run<Bn254, GA_G1>(Ctx*, const void*, size_t, int, const void*, uint64_t, unsigned, void*, uint64_t*, int, uint64_t);
}  // namespace ga

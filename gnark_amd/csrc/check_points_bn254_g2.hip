// Explicit instantiation: batch curve and subgroup checks, bn254 G2 (see check_points.hip.h).
#include "check_points.hip.h"
namespace ga {
template int check_points_run<Bn254, GA_G2>(Ctx*, const void*, size_t, unsigned, uint8_t*, uint64_t*, int, uint64_t);
template int check_points_resident<Bn254, GA_G2>(Ctx*, hipStream_t, const void*, uint64_t, uint64_t, int, int);
template int check_points_tally<Bn254, GA_G2>(Ctx*, hipStream_t, uint64_t*, int*);
}  // namespace ga

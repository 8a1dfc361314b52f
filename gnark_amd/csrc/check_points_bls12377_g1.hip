// Explicit instantiation: batch curve and subgroup checks, bls12377 G1 (see check_points.hip.h).
#include "check_points.hip.h"
namespace ga {
template int check_points_run<Bls12377, GA_G1>(Ctx*, const void*, size_t, unsigned, uint8_t*, uint64_t*, int, uint64_t);
template int check_points_resident<Bls12377, GA_G1>(Ctx*, hipStream_t, const void*, uint64_t, uint64_t, int, int);
template int check_points_tally<Bls12377, GA_G1>(Ctx*, hipStream_t, uint64_t*, int*);
}  // namespace ga

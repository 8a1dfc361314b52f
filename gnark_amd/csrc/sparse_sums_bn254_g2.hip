// Explicit instantiation: sparse point sums, bn254 G2 (see sparse_sums.hip.h).
#include "sparse_sums.hip.h"
namespace ga {
template int sparse_sums_run<Bn254, GA_G2>(Ctx*, const void*, size_t, const uint64_t*, size_t, const uint32_t*, const void*, size_t, unsigned, void*, uint64_t*,
                                           uint64_t, uint32_t, int);
}  // namespace ga

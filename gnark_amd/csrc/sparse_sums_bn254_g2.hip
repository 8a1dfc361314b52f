// Explicit instantiation: sparse point sums, bn254 G2 (see sparse_sums.hip.h).
#include "sparse_sums.hip.h"
namespace ga {
GA_INSTANTIATE_SPARSE_SUMS(Bn254, GA_G2)
}  // namespace ga

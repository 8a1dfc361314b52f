// Explicit instantiation: sparse point sums, bls12381 G2 (see sparse_sums.hip.h).
#include "sparse_sums.hip.h"
namespace ga {
GA_INSTANTIATE_SPARSE_SUMS(Bls12381, GA_G2)
}  // namespace ga

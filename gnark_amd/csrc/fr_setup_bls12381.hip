// Explicit instantiation: the Fr vector calls of groth16.Setup's scalar side, bls12381 (see fr_sparse.hip.h, fr_setup.hip.h).
#include "fr_setup.hip.h"
#include "fr_sparse.hip.h"
namespace ga {
GA_INSTANTIATE_FR_SPARSE(Bls12381)
GA_INSTANTIATE_FR_SETUP(Bls12381)
}  // namespace ga

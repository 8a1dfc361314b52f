// Explicit instantiation: the Fr vector calls of groth16.Setup's scalar side, bn254 (see fr_sparse.hip.h, fr_setup.hip.h).
#include "fr_setup.hip.h"
#include "fr_sparse.hip.h"
namespace ga {
GA_INSTANTIATE_FR_SPARSE(Bn254)
GA_INSTANTIATE_FR_SETUP(Bn254)
}  // namespace ga

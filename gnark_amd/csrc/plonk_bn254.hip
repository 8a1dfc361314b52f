// Explicit instantiation: PLONK quotient / grand product / batch inversion, bn254 (see plonk.hip.h, plonk_batch.hip.h).
#include "plonk_batch.hip.h"
namespace ga {
GA_INSTANTIATE_PLONK(Bn254)
}  // namespace ga

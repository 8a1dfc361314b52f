// Explicit instantiation: PLONK quotient / grand product / batch inversion, bls12377 (see plonk.hip.h, plonk_batch.hip.h).
#include "plonk_batch.hip.h"
namespace ga {
GA_INSTANTIATE_PLONK(Bls12377)
}  // namespace ga

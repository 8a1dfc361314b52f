// Explicit instantiation: mpcsetup's lagrangeCoeffsG2 (the inverse FFT over G2 points), bn254 (see ec_ntt.hip.h).
#include "ec_ntt.hip.h"
namespace ga {
GA_INSTANTIATE_EC_NTT(Bn254, GA_G2)
}  // namespace ga

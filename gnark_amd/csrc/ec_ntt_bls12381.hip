// Explicit instantiation: kzg.ToLagrangeG1 (the inverse FFT over G1 points), bls12381 (see ec_ntt.hip.h).
#include "ec_ntt.hip.h"
namespace ga {
GA_INSTANTIATE_EC_NTT(Bls12381, GA_G1)
}  // namespace ga

// Explicit instantiation: kzg.ToLagrangeG1 (the inverse FFT over G1 points), bn254 (see ec_ntt.hip.h).
#include "ec_ntt.hip.h"
namespace ga {
GA_INSTANTIATE_EC_NTT(Bn254, GA_G1)
}  // namespace ga

// Explicit instantiation: kzg.ToLagrangeG1 (the inverse FFT over G1 points), bn254 (see ec_ntt.hip.h).
#include "ec_ntt.hip.h"
namespace ga {
template int ec_ntt_to_lagrange<Bn254, GA_G1>(Ctx*, const void*, size_t, unsigned, void*, int);
}  // namespace ga

// Explicit instantiation: kzg.ToLagrangeG1 (the inverse FFT over G1 points), bls12377 (see ec_ntt.hip.h).
#include "ec_ntt.hip.h"
namespace ga {
template int ec_ntt_to_lagrange<Bls12377, GA_G1>(Ctx*, const void*, size_t, unsigned, void*, int);
}  // namespace ga

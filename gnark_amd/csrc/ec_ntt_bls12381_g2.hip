// Explicit instantiation: mpcsetup's lagrangeCoeffsG2 (the inverse FFT over G2 points), bls12381 (see ec_ntt.hip.h).
#include "ec_ntt.hip.h"
namespace ga {
template int ec_ntt_to_lagrange<Bls12381, GA_G2>(Ctx*, const void*, size_t, unsigned, void*, int);
}  // namespace ga

// Explicit instantiation: pairing products, bn254 (see pairing.hip.h).
#include "pairing.hip.h"
namespace ga {
template int pairing_run<Bn254>(Ctx*, const void*, const void*, size_t, const uint64_t*, size_t, unsigned, uint8_t*, void*, uint64_t*, uint64_t);
}  // namespace ga

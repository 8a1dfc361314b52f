// Explicit instantiation: the Fr vector calls of groth16.Setup's scalar side, bn254 (see fr_sparse.hip.h, fr_setup.hip.h).
#include "fr_setup.hip.h"
#include "fr_sparse.hip.h"
namespace ga {
template int fr_sparse_run<Bn254>(Ctx*, const void*, size_t, const uint64_t*, size_t, const uint32_t*, const void*, size_t, const uint8_t*, const void*, size_t,
                               unsigned, void*, uint32_t);
template int fr_lagrange_run<Bn254>(Ctx*, int, const void*, size_t, unsigned, void*);
template int fr_compact_run<Bn254>(Ctx*, const void*, size_t, unsigned, void*, uint8_t*, uint64_t*);
template int fr_powers_run<Bn254>(Ctx*, const void*, uint64_t, size_t, unsigned, void*);
}  // namespace ga

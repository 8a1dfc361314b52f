// Explicit instantiation: fixed-base batch scalar multiplication, bn254 G2 (see fixed_base.hip.h).
#include "fixed_base.hip.h"
namespace ga {
template int fixed_base_run<Bn254, GA_G2>(Ctx*, const void*, const void*, size_t, unsigned, void*, int, uint64_t);
}  // namespace ga

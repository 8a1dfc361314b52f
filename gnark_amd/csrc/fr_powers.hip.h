// The geometric progression c * t^e over Fr, one term per lane: what ga_scale_points generates for GA_SCALE_POWERS (the c tau^i of
// SrsCommons.update, phase1.go:104-147) and what ga_fr_powers writes out as a vector (the Z scalars tau^i (tau^n - 1) / delta of
// groth16.Setup, setup.go:181-192; the powers of tau of kzg.NewSRS).  pow_u64 is 64 Fr squarings at most, so there is no prefix scan.
#pragma once
#include "field.hip.h"

namespace ga {

// a field element as the ABI takes it -> canonical, below r: a Montgomery image is converted, a canonical value reduced
template <class FrP>
GA_HD Fe<FrP> fr_canonical(Fe<FrP> s, int mont) {
    if (mont) return from_mont(s);
#pragma unroll 1
    for (int k = 0; k < canonical_steps<FrP>(); k++) reduce_once<FrP>(s.l);   // any 256-bit integer: below r (field.hip.h)
    return s;
}

// c * t^e, canonical; c and t as the ABI takes them
template <class FrP>
GA_HD Fe<FrP> fr_power_term(const Fe<FrP>& c, const Fe<FrP>& t, int mont, uint64_t e) {
    return from_mont(mul(to_mont(fr_canonical(c, mont)), pow_u64(to_mont(fr_canonical(t, mont)), e)));
}

}  // namespace ga

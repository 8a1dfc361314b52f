"""BLS12-377, the G1 / Fr side: the one place the curve's literals live.  tools/gen_constants.py (product header), tools/lazy_bounds.py
and the tests import them from here; the oracle (oracle/pyref.py, oracle/oracle_constants.h) knows two curves and is not touched.

Sources.  p and r: std/math/emulated/emparams/emparams.go:198,213 of the reference; the seed x0: std/algebra/native/sw_bls12377/
pairing.go:365.  The reference does not hold gnark-crypto, so the G1 generator, FrMultiplicativeGen = 22 and the 2-adicity 47 are
restated from gnark-crypto's published bls12-377 package and could not be pinned to a file of the reference; `verify()` checks what
can be checked from the numbers alone (tests/test_bls12_377.py runs it):
  * r = x0^4 - x0^2 + 1 and p = (x0 - 1)^2 r / 3 + x0 (the BLS12 family polynomials);
  * the generator is on y^2 = x^3 + 1, [r]G = O and [(x0 - 1)^2 / 3]G != O;
  * 22 generates Fr*: 22^((r-1)/q) != 1 for every prime q of r - 1 = x0^2 (x0 - 1)(x0 + 1)
    = 2^47 * 3 * 5 * 7 * 13 * 499 * 958612291309063373 * x0^2 (x0 is prime; the list below multiplies back to r - 1).
Nothing interoperable rests on the generator (synthetic bases only); the PLONK coset does rest on FR_GEN.

G2, the pairing and Groth16 on this curve need Fp2 = Fp[u]/(u^2 + 5); the library's Fp2 is u^2 + 1, so none of them is built."""

P = 0x1ae3a4617c510eac63b05c06ca1493b1a22d9f300f5138f1ef3622fba094800170b5d44300000008508c00000000001
R = 8444461749428370424248824938781546531375899335154063827935233455917409239041
SEED = 0x8508c00000000001          # x0
B = 1                              # G1: y^2 = x^3 + 1
G1 = (0x008848defe740a67c8fc6225bf87ff5485951e2caa9d41bb188282c8bd37cb5cd5481512ffcd394eeab9b16eb21be9ef,
      0x01914a69c5102eff1f674f5d30afeec4bd7fb348ca3e52d96d182ad44fb82305c2fe3d3634a9591afd82de55559c8ea6)
G1_COFACTOR = (SEED - 1) ** 2 // 3
FR_GEN = 22                        # fft.Domain.FrMultiplicativeGen
FR_ADICITY = 47
# the primes of r - 1 = x0^2 (x0 - 1)(x0 + 1), x0 itself among them
FR_MINUS_ONE_PRIMES = (2, 3, 5, 7, 13, 499, 958612291309063373, SEED)
NAME, CID, FP_LIMBS, FR_LIMBS = "bls12-377", 2, 6, 4
LAZY = (P, 28, 14, 377)            # tools/lazy_bounds.py: modulus, limb bits, limbs, bit length (the radix BLS12-381's Fp has)


def curve():
    """pyref.Curve for this curve, built outside the oracle.  b2 / g2 are None: pyref's G2 arithmetic is u^2 + 1 and must not be
    reached (g2_group, the pairing and Groth16 of pyref raise on them)."""
    import pyref
    return pyref.Curve(name=NAME, cid=CID, p=P, r=R, fp_limbs=FP_LIMBS, fr_limbs=FR_LIMBS, b=B, b2=None, g1=G1, g2=None,
                       fr_gen=FR_GEN, fr_adicity=FR_ADICITY)


def beta():
    """The cube root of unity of Fp with P + [x0^2] phi(P) = O on the generator, phi(x, y) = (BETA x, y): chosen, as for BLS12-381,
    by that identity (check_points.hip.h tests subgroup membership with it)."""
    import pyref
    G = pyref.Group(pyref.FpOps(P), B)
    g = next(g for g in range(2, 100) if pow(g, (P - 1) // 3, P) != 1)
    w = pow(g, (P - 1) // 3, P)
    ok = [b for b in (w, w * w % P) if G.add(G1, G.mul((b * G1[0] % P, G1[1]), SEED * SEED)) is None]
    assert len(ok) == 1, "exactly one cube root of unity satisfies P + [x0^2] phi(P) = O on the generator"
    return ok[0]


def verify():
    import pyref
    x0 = SEED
    assert R == x0 ** 4 - x0 ** 2 + 1 and 3 * (P - x0) == (x0 - 1) ** 2 * R
    assert P.bit_length() == 377 and R.bit_length() == 253
    G = pyref.Group(pyref.FpOps(P), B)
    assert G.on_curve(G1) and G.mul(G1, R) is None and G.mul(G1, G1_COFACTOR) is not None
    m = R - 1
    for q in FR_MINUS_ONE_PRIMES:
        assert m % q == 0
        while m % q == 0:
            m //= q
        assert pow(FR_GEN, (R - 1) // q, R) != 1, q
    assert m == 1, "the prime list does not multiply back to r - 1"
    assert (R - 1) % (1 << FR_ADICITY) == 0 and (R - 1) >> FR_ADICITY & 1
    return True

#!/usr/bin/env python3
"""Generate the field / curve constant headers from the moduli.

  gnark_amd/csrc/constants.h   product header, 32-bit limbs (device arithmetic uses v_mad_u64_u32)
  oracle/oracle_constants.h    oracle header, 64-bit limbs (plain C, unsigned __int128)

Moduli sources in the reference: backend/groth16/bn254/solidity.go:64-65,
std/math/emulated/emparams/emparams.go:142-157,225-241; BLS12-377 (product header only, G1 / Fr): tools/bls12_377_params.py.  Everything else (R, R^2, -p^-1,
roots of unity) is derived here from the moduli.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from pyref import BN254, BLS12_381, Fp2Ops, Fp12Ops, g1_group, g2_group  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bls12_377_params as BLS12_377  # noqa: E402

# the curves' seeds (x0 of the BN / BLS12 families): p, r and the cofactors are polynomials in them
BN254_SEED = 4965661367192848881
BLS12_381_SEED = -0xd201000000010000


def limbs(x, n, w):
    return [(x >> (w * i)) & ((1 << w) - 1) for i in range(n)]


def arr(x, n, w):
    sfx = "u" if w == 32 else "ull"
    return "{" + ", ".join(f"0x{v:0{w // 4}x}{sfx}" for v in limbs(x, n, w)) + "}"


FP2_LAZY_K = 16   # operands of the lazy Fp2 product are below 16p (asserted by tools/lazy_bounds.py)


def fp2_lazy_offset(mod, n64, K=FP2_LAZY_K):
    """Column constants Z[0..2NL-2] for field29.hip.h's Fp2 product: a multiple of p in a redundant base-2^L representation whose
    every column dominates the corresponding column of a1*b1 (operands < K*p, normalized limbs), so that
    a0*b0 - a1*b1 + Z can be formed column by column in unsigned 64-bit arithmetic before ONE Montgomery reduction."""
    n32 = 2 * n64
    L = 29 if n32 == 8 else 28
    NL = (32 * n32 + L - 1) // L + (1 if (32 * n32) % L == 0 else 0)
    top = (K * mod >> (L * (NL - 1))) + 1
    A = [2 ** L - 1] * (NL - 1) + [top]
    ncol = 2 * NL - 1
    colb = [sum(A[i] * A[j - i] for i in range(NL) if 0 <= j - i < NL) for j in range(ncol)]
    t = [0] * ncol            # t[j]: units of 2^L column j borrows from column j+1
    prev = 0
    for j in range(ncol - 1):
        t[j] = (colb[j] + prev + (1 << L) - 1) >> L
        prev = t[j]
    need_top = colb[ncol - 1] + prev
    zint = -(-(need_top << (L * (ncol - 1))) // mod) * mod
    z = [(zint >> (L * j)) & ((1 << L) - 1) for j in range(ncol - 1)] + [zint >> (L * (ncol - 1))]
    Z = [z[j] + (t[j] << L) - (t[j - 1] if j else 0) for j in range(ncol)]
    assert sum(Z[j] << (L * j) for j in range(ncol)) == zint and zint % mod == 0
    assert all(Z[j] >= colb[j] for j in range(ncol)) and max(Z) + max(colb) + NL * (1 << (2 * L)) < 1 << 63
    R = 1 << (L * NL)
    return Z, zint, -(-zint // R)     # the offset adds less than this to a reduced value


def field_block(name, mod, n64, w, extra=None, fp2=True):
    n = n64 * (64 // w)
    R = 1 << (64 * n64)
    ty = "uint32_t" if w == 32 else "uint64_t"
    inv = (-pow(mod, -1, 1 << w)) % (1 << w)
    out = [f"struct {name} {{"]
    out.append(f"    static constexpr int N = {n};          // {w}-bit limbs")
    out.append(f"    static constexpr int N64 = {n64};")
    out.append(f"    static constexpr int BITS = {mod.bit_length()};")
    out.append(f"    static constexpr {ty} INV = 0x{inv:x}{'u' if w == 32 else 'ull'};   // -mod^-1 mod 2^{w}")
    out.append(f"    static constexpr {ty} MOD[{n}] = {arr(mod, n, w)};")
    out.append(f"    static constexpr {ty} ONE[{n}] = {arr(R % mod, n, w)};   // R mod p")
    out.append(f"    static constexpr {ty} R2[{n}] = {arr(R * R % mod, n, w)};    // R^2 mod p")
    out.append(f"    static constexpr {ty} PM2[{n}] = {arr(mod - 2, n, w)};   // p-2 (Fermat inverse exponent)")
    out.append(f"    static constexpr uint32_t MU12 = {(1 << (mod.bit_length() + 8)) // mod}u;   // floor(2^(BITS+8) / p): Barrett quotient estimate (field29.hip.h)")
    if w == 32 and name.endswith("_Fp") and fp2:
        Z, zint, add = fp2_lazy_offset(mod, n64)
        out.append(f"    // lazy Fp2 product (field29.hip.h): redundant-digit columns of a multiple of p dominating a1*b1 for operands < {FP2_LAZY_K}p;")
        out.append(f"    // it adds < {add / mod:.3f} p to the reduced real part")
        out.append(f"    static constexpr int FP2Z_K = {FP2_LAZY_K};")
        out.append(f"    static constexpr uint64_t FP2Z[{len(Z)}] = {{" + ", ".join(f"0x{v:x}ull" for v in Z) + "};")
    elif w == 32 and name.endswith("_Fp"):
        # the G1 kernels name the constant in `Lazy<F>::FP2 ? P::FP2Z_K : 8` and never select it; the column table FP2Z, which the Fp2
        # product needs, stays out: an Fe2 over this field does not compile
        out.append(f"    static constexpr int FP2Z_K = {FP2_LAZY_K};   // named, never selected: there is no Fp2 over this field (no FP2Z)")
    for k, v in (extra or {}).items():
        if isinstance(v, int) and k.isupper() and k.startswith("I_"):
            out.append(f"    static constexpr int {k[2:]} = {v};")
        elif isinstance(v, list):
            rows = ", ".join(arr(x * R % mod, n, w) for x in v)
            out.append(f"    static constexpr {ty} {k}[{len(v)}][{n}] = {{{rows}}};   // Montgomery form")
        else:
            out.append(f"    static constexpr {ty} {k}[{n}] = {arr(v * R % mod, n, w)};   // Montgomery form")
    out.append("};")
    return "\n".join(out)


def c_field_block(name, mod, n64, extra=None):
    """plain-C flavour for the oracle (no structs with static members)."""
    R = 1 << (64 * n64)
    inv = (-pow(mod, -1, 1 << 64)) % (1 << 64)
    out = [f"#define {name}_N {n64}", f"#define {name}_BITS {mod.bit_length()}",
           f"static const uint64_t {name}_INV = 0x{inv:x}ull;",
           f"static const uint64_t {name}_MOD[{n64}] = {arr(mod, n64, 64)};",
           f"static const uint64_t {name}_ONE[{n64}] = {arr(R % mod, n64, 64)};",
           f"static const uint64_t {name}_R2[{n64}] = {arr(R * R % mod, n64, 64)};"]
    for k, v in (extra or {}).items():
        if k.startswith("I_"):
            out.append(f"#define {name}_{k[2:]} {v}")
        else:
            out.append(f"static const uint64_t {name}_{k}[{n64}] = {arr(v * R % mod, n64, 64)};")
    return "\n".join(out)


def fp2_pow(F, a, e):
    r = F.one
    while e:
        if e & 1:
            r = F.mul(r, a)
        a = F.mul(a, a)
        e >>= 1
    return r


def endo_constants(c):
    """The constants of check_points.hip.h (product header only), every one chosen by the identity it serves on the generator:
    BLS12-381: BETA, the cube root of unity with P + [x0^2] phi(P) = O for phi(x, y) = (BETA x, y), and PSI_X / PSI_Y, the
    coefficients of the untwist-Frobenius-twist psi(x, y) = (conj(x) PSI_X, conj(y) PSI_Y) with psi(P) = [x0] P;
    BN254: PSI_X / PSI_Y, and psi^2, psi^3 folded: psi^2(x, y) = (x PSI2_X, y PSI2_Y), psi^3(x, y) = (conj(x) PSI3_X, conj(y) PSI3_Y),
    with [x0 + 1] P + psi([x0] P) + psi^2([x0] P) = psi^3([2 x0] P)."""
    p = c.p
    F2, G1, G2 = Fp2Ops(p), g1_group(c), g2_group(c)
    conj = lambda a: (a[0], (-a[1]) % p)
    out = {}
    if c is BLS12_381:
        x0, xi, sign = BLS12_381_SEED, (1, 1), -1
        g = next(g for g in range(2, 100) if pow(g, (p - 1) // 3, p) != 1)
        w = pow(g, (p - 1) // 3, p)
        ok = [b for b in (w, w * w % p) if G1.add(c.g1, G1.mul((b * c.g1[0] % p, c.g1[1]), x0 * x0)) is None]
        assert len(ok) == 1, "exactly one cube root of unity satisfies P + [x0^2] phi(P) = O on the generator"
        out["BETA"] = ok[0]
    else:
        x0, xi, sign = BN254_SEED, (9, 1), 1
    cx, cy = fp2_pow(F2, xi, (p - 1) // 3), fp2_pow(F2, xi, (p - 1) // 2)
    if sign < 0:
        cx, cy = F2.inv(cx), F2.inv(cy)
    psi = lambda P: None if P is None else (F2.mul(conj(P[0]), cx), F2.mul(conj(P[1]), cy))
    assert G2.on_curve(psi(c.g2))
    out.update(PSI_X0=cx[0], PSI_X1=cx[1], PSI_Y0=cy[0], PSI_Y1=cy[1])
    if c is BLS12_381:
        assert psi(c.g2) == G2.mul(c.g2, x0)
    else:
        nx, ny = F2.mul(cx, conj(cx)), F2.mul(cy, conj(cy))
        assert nx[1] == 0 and ny[1] == 0
        c3x, c3y = F2.mul(nx, cx), F2.mul(ny, cy)
        psi2 = lambda P: (F2.mul(P[0], nx), F2.mul(P[1], ny))
        psi3 = lambda P: (F2.mul(conj(P[0]), c3x), F2.mul(conj(P[1]), c3y))
        Q = G2.mul(c.g2, x0)
        assert psi2(Q) == psi(psi(Q)) and psi3(Q) == psi(psi2(Q))
        assert G2.add(G2.add(G2.add(Q, c.g2), psi(Q)), psi2(Q)) == psi3(G2.add(Q, Q))
        out.update(PSI2_X=nx[0], PSI2_Y=ny[0], PSI3_X0=c3x[0], PSI3_X1=c3x[1], PSI3_Y0=c3y[0], PSI3_Y1=c3y[1])
    return out


def pairing_constants(c):
    """The Frobenius constants of pairing.hip.h (product header only): in Fp12 = Fp2[w]/(w^6 - xi) the p^k-power Frobenius sends
    a w^i (a in Fp2) to a^(p^k) g w^i with g = xi^(i (p^k - 1)/6).  FROB1 / FROB3: rows 2(i-1), 2(i-1)+1 are the two Fp halves of g
    for k = 1 / 3 and i = 1..5; FROB2: row i-1 is g for k = 2, which lies in Fp.  Each is asserted against the p^k-th power of w^i
    in plain integer polynomial arithmetic (pyref.Fp12Ops)."""
    p = c.p
    F2, F12 = Fp2Ops(p), Fp12Ops(c)
    xi = (F12.a, 1)
    out = {"FROB1": [], "FROB2": [], "FROB3": []}
    for k in (1, 2, 3):
        for i in range(1, 6):
            g = fp2_pow(F2, xi, i * (p ** k - 1) // 6)
            wi = [0] * 12
            wi[i] = 1
            assert F12.pow(wi, p ** k) == F12.embed_fp2(g, i), (c.name, k, i)
            if k == 2:
                assert g[1] == 0
                out["FROB2"].append(g[0])
            else:
                out["FROB%d" % k] += [g[0], g[1]]
    return out


def main(prod_path=None, oracle_path=None):
    """writes the two headers in place; the tests pass other paths and compare"""
    hdr = ["// GENERATED by tools/gen_constants.py -- do not edit.", "#pragma once", "#include <stdint.h>", ""]
    prod = list(hdr) + ["namespace ga {", ""]
    orc = list(hdr)
    for c, tag in ((BN254, "BN254"), (BLS12_381, "BLS12_381")):
        wmax = c.fr_root_of_unity(1 << c.fr_adicity)
        fr_extra = {"ROOT": wmax, "ROOT_INV": pow(wmax, -1, c.r), "GEN": c.fr_gen,
                    "GEN_INV": pow(c.fr_gen, -1, c.r), "I_ADICITY": c.fr_adicity}
        fp_extra = {"G1X": c.g1[0], "G1Y": c.g1[1], "G2X0": c.g2[0][0], "G2X1": c.g2[0][1],
                    "G2Y0": c.g2[1][0], "G2Y1": c.g2[1][1], "B1": c.b, "B2_0": c.b2[0], "B2_1": c.b2[1]}
        prod.append(field_block(f"{tag}_Fp", c.p, c.fp_limbs, 32, {**fp_extra, **endo_constants(c), **pairing_constants(c)}))
        prod.append("")
        prod.append(field_block(f"{tag}_Fr", c.r, c.fr_limbs, 32, fr_extra))
        prod.append("")
        orc.append(c_field_block(f"{tag}_FP", c.p, c.fp_limbs, fp_extra))
        orc.append("")
        orc.append(c_field_block(f"{tag}_FR", c.r, c.fr_limbs, fr_extra))
        orc.append("")
    # BLS12-377, product header only, G1 and Fr only: no G2*, B2*, PSI*, FROB* and no FP2Z -- the library's Fp2 is Fp[u]/(u^2 + 1) and this
    # curve's is u^2 + 5, so no Fe2 / G2 / pairing template may be instantiated over BLS12_377_Fp (a missing constant is a compile error)
    q = BLS12_377
    wmax = pow(q.FR_GEN, (q.R - 1) >> q.FR_ADICITY, q.R)
    prod.append(field_block("BLS12_377_Fp", q.P, q.FP_LIMBS, 32, {"G1X": q.G1[0], "G1Y": q.G1[1], "B1": q.B, "BETA": q.beta()}, fp2=False))
    prod.append("")
    prod.append(field_block("BLS12_377_Fr", q.R, q.FR_LIMBS, 32, {"ROOT": wmax, "ROOT_INV": pow(wmax, -1, q.R), "GEN": q.FR_GEN,
                                                                  "GEN_INV": pow(q.FR_GEN, -1, q.R), "I_ADICITY": q.FR_ADICITY}))
    prod.append("")
    prod.append("}  // namespace ga")
    with open(prod_path or os.path.join(ROOT, "gnark_amd", "csrc", "constants.h"), "w") as f:
        f.write("\n".join(prod) + "\n")
    with open(oracle_path or os.path.join(ROOT, "oracle", "oracle_constants.h"), "w") as f:
        f.write("\n".join(orc) + "\n")
    print("wrote constants.h, oracle_constants.h")


if __name__ == "__main__":
    main()

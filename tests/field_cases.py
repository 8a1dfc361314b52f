"""Boundary-value cases for the field layer (field.hip.h, field29.hip.h) and the point formulas on it (msm_lazy.hip.h,
msm_bucket.hip.h), run through the test-only probe tests/probe/field_probe.hip.  One set of case functions; tests/test_field_boundaries.py
runs them against the emulation build of the probe, tests/test_field_boundaries_gpu.py against the gfx950 build.

The reference is plain Python integers: R = 2^(32N) (the memory format's Montgomery radix), R' = 2^(NL*L) (the lazy representation's),
pyref's group law for points.  Nothing here is computed with the code under test."""
import ctypes
import functools
import math
import os
import sys

import numpy as np

import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bls12_377_params  # noqa: E402
import lazy_bounds  # noqa: E402

# op codes of tests/probe/field_probe.hip
(OP_ADD, OP_SUB, OP_NEG, OP_DBL, OP_MUL, OP_SQR, OP_INV, OP_FROM_MONT, OP_TO_MONT, OP_MUL_SMALL) = range(10)
(OP_F29_FROM_MEM, OP_F29_UNPACK, OP_F29_HAT_PACKED, OP_F29_TO_MEM, OP_F29_PACK_CANONICAL, OP_F29_PACK_HAT) = range(10, 16)
(OP_F29_NORMALIZE, OP_F29_ADD, OP_F29_ADD_RAW, OP_F29_SUB, OP_F29_SUB_RAW, OP_F29_SUB_WIDE, OP_F29_MUL, OP_F29_SQR, OP_F29_MUL_SUB,
 OP_F29_PARTIAL_REDUCE, OP_F29_REDUCE_3P, OP_F29_IS_ZERO_MOD_P, OP_F29_INV) = range(20, 33)
(OP_F29X2_MUL, OP_F29X2_SQR, OP_F29X2_MUL_SUB, OP_F29X2_INV) = range(40, 44)
(OP_PT_ADD29, OP_PT_DBL29, OP_PT_MADD29, OP_PT_MDBL29, OP_PT_MADD29_COMPLETE) = range(50, 55)
OP_DIGIT_WALK, DIGIT_WINDOWS = 70, 64
OP_PT2 = 10   # added to a point op: the same formula over Fp2
FP2Z_K = 16   # constants.h: the negation constant of the lazy Fp2 product, both curves that have an Fp2


class Field:
    def __init__(self, idx, name, p, curve=None, has_fp2=None):
        self.idx, self.name, self.p, self.curve = idx, name, p, curve
        self.bits = p.bit_length()
        self.N = (self.bits + 63) // 64 * 2                 # 32-bit words of the memory image
        self.L = 29 if self.N == 8 else 28                  # field.hip.h Radix<P>
        self.NL = (32 * self.N + self.L - 1) // self.L + (1 if (32 * self.N) % self.L == 0 else 0)
        self.R = 1 << (32 * self.N)
        self.Rp = 1 << (self.NL * self.L)
        self.S = self.NL * self.L - 32 * self.N
        self.mask = (1 << self.L) - 1
        self.unit = 1 << (self.L * (self.NL - 1))           # one unit of the top limb
        self.is_base = curve is not None
        # Fp2 = Fp[u]/(u^2 + 1) is built over the field: F29x2, the G2 point formulas, FP2Z_K (not over BLS12-377's Fp)
        self.has_fp2 = self.is_base if has_fp2 is None else has_fp2
        assert self.is_base or not self.has_fp2

    def __repr__(self):
        return self.name


FIELDS = {
    "bn254_fp": Field(0, "bn254_fp", pyref.BN254.p, "bn254"),
    "bn254_fr": Field(1, "bn254_fr", pyref.BN254.r),
    "bls12_381_fp": Field(2, "bls12_381_fp", pyref.BLS12_381.p, "bls12-381"),
    "bls12_381_fr": Field(3, "bls12_381_fr", pyref.BLS12_381.r),
    "bls12_377_fp": Field(4, "bls12_377_fp", bls12_377_params.P, "bls12-377", has_fp2=False),
    "bls12_377_fr": Field(5, "bls12_377_fr", bls12_377_params.R),
}
BASE_FIELDS = [n for n, f in FIELDS.items() if f.is_base]
FP2_FIELDS = [n for n, f in FIELDS.items() if f.has_fp2]
# (field, fp2) of every point-formula run: G1 over each base field, G2 where the field has an Fp2
POINT_FIELDS = [(n, fp2) for n in BASE_FIELDS for fp2 in (False, True) if not fp2 or FIELDS[n].has_fp2]

# pyref.CURVES knows the oracle's two curves; BLS12-377 is built outside it (tools/bls12_377_params.py), G1 / Fr side only
BLS12_377 = bls12_377_params.curve()
CURVE_BY_NAME = dict(pyref.CURVES, **{BLS12_377.name: BLS12_377})


def fp_of(c):
    """the base field of a curve"""
    return next(f for f in FIELDS.values() if f.curve == c.name)


def fr_of(c):
    """the scalar field of a curve"""
    return next(f for f in FIELDS.values() if not f.is_base and f.p == c.r)


# ---- the probe ------------------------------------------------------------------------------------------------------------------
class Probe:
    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.fn = self.lib.ga_probe_run
        self.fn.restype = ctypes.c_int
        self.fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p,
                            ctypes.c_size_t]

    def run(self, f, op, rows, out_words, k=0):
        """rows: n equal-length lists of 32-bit words -> n lists of out_words words (Python ints)"""
        a = np.ascontiguousarray(np.array(rows, dtype=np.uint64).astype(np.uint32))
        assert a.ndim == 2 and len(rows) <= 40000, a.shape
        out = np.zeros((a.shape[0], out_words), dtype=np.uint32)
        rc = self.fn(f.idx, op, k, a.ctypes.data, a.shape[0], a.shape[1], out.ctypes.data, out_words)
        assert rc == 0, "ga_probe_run(field=%s, op=%d, k=%d) returned %d" % (f, op, k, rc)
        return out.tolist()


# ---- words and limbs ------------------------------------------------------------------------------------------------------------
def words(f, v):
    assert 0 <= v < f.R
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(f.N)]


def limbs(f, v):
    """normalized limbs; the top limb keeps the excess"""
    assert 0 <= v < (1 << (f.L * (f.NL - 1) + 32))
    return [(v >> (f.L * i)) & f.mask for i in range(f.NL - 1)] + [v >> (f.L * (f.NL - 1))]


def wval(row):
    return sum(int(w) << (32 * i) for i, w in enumerate(row))


def lval(f, row):
    return sum(int(w) << (f.L * i) for i, w in enumerate(row))


def assert_normalized(f, row, what):
    assert all(w <= f.mask for w in row[:-1]), (what, "a limb below the top exceeds 2^L - 1", row)
    assert row[-1] < (1 << 31), (what, "the top limb wrapped (a borrow)", row)


# ---- operand sets ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def extremes(f):
    """~20 canonical values at the edges; as raw words every pattern is present itself AND as a Montgomery image"""
    p, R = f.p, f.R
    Ri = pow(R, -1, p)
    top_ones = (1 << (f.bits - 1)) - 1                      # all limbs 2^L - 1, truncated below p
    pats = [1, 0xFFFFFFFF, 0xFFFFFFFF << 32 * (f.N - 2), f.mask, f.mask << f.L * (f.NL - 2), top_ones, p - 1]
    vals = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, R % p, Ri, 1 << (f.bits - 1), top_ones, (1 << 32) - 1, f.mask, 1 << f.L]
    vals += [x % p for x in pats] + [x * Ri % p for x in pats]
    return tuple(dict.fromkeys(vals))


@functools.lru_cache(maxsize=None)
def canon(f):
    """the deterministic operand set: a few hundred canonical values"""
    p, R = f.p, f.R
    Ri = pow(R, -1, p)
    vals = list(extremes(f))
    ks = sorted({k for k in range(0, f.bits + 1) if k % 32 == 0 or k % f.L == 0})
    for k in ks:
        vals += [x for x in ((1 << k), (1 << k) - 1) if 0 <= x < p]
    pats = [0xFFFFFFFF << (32 * w) for w in range(f.N)] + [f.mask << (f.L * i) for i in range(f.NL)]
    vals += [x * Ri % p for x in pats if x < p]              # values whose Montgomery image is the pattern
    rng = pyref.Xoshiro(0xB0DA + f.idx)
    vals += [rng.field(p) for _ in range(64)]
    vals += [v * R % p for v in list(vals)]                  # ... and every value's own image, for the functions that take raw words
    return tuple(dict.fromkeys(vals))


def lifts(f, v, limit=None, ks=(0, 1, 2, 3)):
    """v + k*p for k in ks and the largest k below limit (default: 2^(NL*L-2), the bound of the lazy representation)"""
    limit = f.Rp // 4 if limit is None else limit
    out = [v + k * f.p for k in ks if v + k * f.p < limit]
    out.append(v + (limit - 1 - v) // f.p * f.p)
    return list(dict.fromkeys(out))


def sample(seq, n, seed):
    seq = list(seq)
    if len(seq) <= n:
        return seq
    rng = pyref.Xoshiro(seed)
    return [seq[rng.next() % len(seq)] for _ in range(n)]


@functools.lru_cache(maxsize=None)
def lazy_pairs(f, blimit=None):
    """pairs (a, b) of lifted values: the full cross product of the lifted extremes' corners and a seeded sample of the rest.
    blimit: b stays below it (the precondition of a subtraction); its lifts are then k = 0, 1 and the two largest that fit"""
    def blifts(v):
        if blimit is None:
            return lifts(f, v)
        top = (blimit - 1 - v) // f.p
        return list(dict.fromkeys(v + k * f.p for k in (0, 1, top - 1, top) if 0 <= k <= top))
    ex = extremes(f)
    A = [x for v in ex for x in (lifts(f, v)[0], lifts(f, v)[-1])] + [lifts(f, v)[1] for v in ex[:6]]
    B = [x for v in ex for x in (blifts(v)[0], blifts(v)[-1])]
    pairs = [(a, b) for a in A for b in B]
    rest_a = [x for v in canon(f) for x in lifts(f, v)]
    rest_b = [x for v in canon(f) for x in blifts(v)]
    rng = pyref.Xoshiro(77 + f.idx)
    pairs += [(rest_a[rng.next() % len(rest_a)], rest_b[rng.next() % len(rest_b)]) for _ in range(3000)]
    if blimit is not None:                                   # the values right at the limit, whatever their residue
        pairs += [(a, b) for a in (0, 1, f.p, A[1]) for b in (blimit - 1, blimit - 2, blimit - f.p)]
    return tuple(pairs)


# ---- packed Fe<P> ---------------------------------------------------------------------------------------------------------------
def case_packed_binary(pr, f):
    ex, cn = extremes(f), canon(f)
    rng = pyref.Xoshiro(5 + f.idx)
    pairs = [(a, b) for a in ex for b in ex] + [(cn[rng.next() % len(cn)], cn[rng.next() % len(cn)]) for _ in range(3000)]
    rows = [words(f, a) + words(f, b) for a, b in pairs]
    Ri = pow(f.R, -1, f.p)
    for op, ref in ((OP_ADD, lambda a, b: (a + b) % f.p), (OP_SUB, lambda a, b: (a - b) % f.p), (OP_MUL, lambda a, b: a * b * Ri % f.p)):
        got = pr.run(f, op, rows, f.N)
        for (a, b), g in zip(pairs, got):
            assert wval(g) == ref(a, b), (f, op, hex(a), hex(b), hex(wval(g)))


def case_packed_unary(pr, f):
    cn = canon(f)
    rows = [words(f, a) for a in cn]
    p, R = f.p, f.R
    Ri = pow(R, -1, p)
    refs = [(OP_NEG, 0, lambda a: -a % p), (OP_DBL, 0, lambda a: 2 * a % p), (OP_SQR, 0, lambda a: a * a * Ri % p),
            (OP_FROM_MONT, 0, lambda a: a * Ri % p), (OP_TO_MONT, 0, lambda a: a * R % p),
            (OP_INV, 0, lambda a: pow(a, p - 2, p) * R * R % p)]
    for k in (0, 1, 2, 3, 5, 13, 0xFFFF, 0x80000000, 0xFFFFFFFF):
        refs.append((OP_MUL_SMALL, k, (lambda k: lambda a: a * k % p)(k)))
    for op, k, ref in refs:
        # (the probe's k is a C int: the factor of mul_small travels as its two's complement)
        got = pr.run(f, op, rows, f.N, k=k - (1 << 32) if k >= (1 << 31) else k)
        for a, g in zip(cn, got):
            assert wval(g) == ref(a), (f, op, k, hex(a), hex(wval(g)))


# ---- conversions ----------------------------------------------------------------------------------------------------------------
def case_conversions(pr, f):
    p, cn = f.p, canon(f)
    rows = [words(f, a) for a in cn]
    hat = pr.run(f, OP_F29_FROM_MEM, rows, f.NL)
    hp = pr.run(f, OP_F29_HAT_PACKED, rows, f.N)
    for a, g, h in zip(cn, hat, hp):
        want = a * (1 << f.S) % p                            # hat = memory value * 2^S
        assert g == limbs(f, want), (f, "from_mem", hex(a))
        assert wval(h) == want, (f, "hat_packed", hex(a))
    # unpack is bit-field extraction of ANY 32N-bit integer: also all-ones and the values just around p and 2^(32N)
    raw = list(cn) + [f.R - 1, f.R - 2, p, p + 1, 2 * p - 1, (1 << (32 * f.N - 1)), f.R - (1 << 32)]
    raw = [v for v in raw if v < f.R]
    got = pr.run(f, OP_F29_UNPACK, [words(f, v) for v in raw], f.NL)
    for v, g in zip(raw, got):
        assert g == limbs(f, v), (f, "unpack", hex(v))
    # to_mem: any normalized value below R' -> canonical memory image; from_mem . to_mem = identity on canonical images
    Si = pow(1 << f.S, -1, p)
    lz = [x for v in cn for x in lifts(f, v) + [lifts(f, v, limit=f.Rp)[-1]]]
    got = pr.run(f, OP_F29_TO_MEM, [limbs(f, v) for v in lz], f.N)
    for v, g in zip(lz, got):
        assert wval(g) == v * Si % p, (f, "to_mem", hex(v), hex(wval(g)))
    back = pr.run(f, OP_F29_TO_MEM, hat, f.N)
    assert [wval(g) for g in back] == list(cn), (f, "from_mem then to_mem is not the identity")
    # pack_canonical: any value below 3p that fits the 32N-bit words -> canonical
    pc = [v + k * p for v in cn for k in (0, 1, 2) if v + k * p < f.R]
    pc += [x for x in (p - 1, p, p + 1, 2 * p - 1, 2 * p, 2 * p + 1, 3 * p - 1, f.R - 1) if x < min(3 * p, f.R)]
    got = pr.run(f, OP_F29_PACK_CANONICAL, [limbs(f, v) for v in pc], f.N)
    for v, g in zip(pc, got):
        assert wval(g) == v % p, (f, "pack_canonical", hex(v), hex(wval(g)))
    # pack_hat: any normalized value below R' -> canonical words of the same domain; where the Barrett step does not reach that far
    # (BLS12-377 Fp), any value below hat_limit
    top = min(f.Rp, hat_limit(f))
    lz = [x for v in cn for x in lifts(f, v, limit=min(f.Rp // 4, top)) + [lifts(f, v, limit=top)[-1]]]
    got = pr.run(f, OP_F29_PACK_HAT, [limbs(f, v) for v in lz], f.N)
    for v, g in zip(lz, got):
        assert wval(g) == v % p, (f, "pack_hat", hex(v), hex(wval(g)))


# ---- lazy F29<P> ----------------------------------------------------------------------------------------------------------------
def case_lazy_add_normalize(pr, f):
    pairs = lazy_pairs(f)
    rows = [limbs(f, a) + limbs(f, b) for a, b in pairs]
    got = pr.run(f, OP_F29_ADD, rows, f.NL)
    raw = pr.run(f, OP_F29_ADD_RAW, rows, f.NL)
    for (a, b), g, r in zip(pairs, got, raw):
        assert_normalized(f, g, "f29_add")
        assert lval(f, g) == a + b, (f, "f29_add", hex(a), hex(b))
        assert r == [x + y for x, y in zip(limbs(f, a), limbs(f, b))], (f, "f29_add_raw", hex(a), hex(b))
    # normalize: limbs up to 2^31 - 1 everywhere (the widest a multiplicand may be), carries through every limb, the top limb
    # keeps the excess
    rng = pyref.Xoshiro(11 + f.idx)
    M31 = (1 << 31) - 1
    un = [[M31] * f.NL, [f.mask] * f.NL, [f.mask + 1] * f.NL, [3 * f.mask] * f.NL, [0] * (f.NL - 1) + [M31], [M31] + [f.mask] * (f.NL - 1),
          [M31] + [f.mask] * (f.NL - 2) + [0]]
    un += [[rng.next() & M31 for _ in range(f.NL)] for _ in range(500)]
    un += [[rng.next() % (3 << f.L) for _ in range(f.NL)] for _ in range(500)]
    got = pr.run(f, OP_F29_NORMALIZE, un, f.NL)
    for u, g in zip(un, got):
        assert all(w <= f.mask for w in g[:-1]) and lval(f, g) == lval(f, u), (f, "f29_normalize", u, g)


def kp_lend_limbs(f, K):
    """K*p as the subtractions add it limb-wise (field29.hip.h kp_limb): the plain limbs of K*p, the top one keeping the overflow, where
    every limb but the top borrows 2^L from its upper neighbour and every limb but the bottom lends 1 to its lower one"""
    plain = limbs(f, K * f.p)
    return [w + ((1 << f.L) if i < f.NL - 1 else 0) - (1 if i > 0 else 0) for i, w in enumerate(plain)]


def case_lazy_sub(pr, f):
    for K in (2, 4, 8):
        pairs = lazy_pairs(f, K * f.p)                       # b < K*p
        rows = [limbs(f, a) + limbs(f, b) for a, b in pairs]
        got = pr.run(f, OP_F29_SUB, rows, f.NL, k=K)
        for (a, b), g in zip(pairs, got):
            assert_normalized(f, g, "f29_sub<%d>" % K)
            assert lval(f, g) == a - b + K * f.p, (f, "f29_sub<%d>" % K, hex(a), hex(b), hex(lval(f, g)))
    for K in (4, 8):
        # without the carry sweep the top limb cannot wait for the loan its lower neighbours repay: b's top limb must be below
        # K*p's (the margin of one top-limb unit that tools/lazy_bounds.py `need` asserts for every subtraction)
        pairs = lazy_pairs(f, K * f.p // f.unit * f.unit)
        rows = [limbs(f, a) + limbs(f, b) for a, b in pairs]
        got = pr.run(f, OP_F29_SUB_RAW, rows, f.NL, k=K)
        for (a, b), g in zip(pairs, got):
            assert all(w < (3 << f.L) for w in g[:-1]) and g[-1] < (1 << 31), (f, "f29_sub_raw: limb out of range", hex(a), hex(b), g)
            assert lval(f, g) == a - b + K * f.p, (f, "f29_sub_raw<%d>" % K, hex(a), hex(b))
            assert g == [x + k - y for x, k, y in zip(limbs(f, a), kp_lend_limbs(f, K), limbs(f, b))], (f, "f29_sub_raw<%d> limbs" % K)


def wide_operands(f):
    """un-normalized b of f29_sub_wide<4, 4>: limb-wise sums x + 2y (the PPP + 2Q of the mixed addition) below 4p, limbs below 3*2^L,
    and the widest: every limb but the top 3*(2^L - 1), the top limb as large as 4p allows"""
    p = f.p
    ex = extremes(f)
    out = []
    for x in ex:
        for y in ex:
            for kx, ky in ((0, 0), (1, 0), (0, 1), (1, 1)):
                xx, yy = x + kx * p, y + ky * p
                if xx + 2 * yy < 4 * p:
                    out.append([a + 2 * b for a, b in zip(limbs(f, xx), limbs(f, yy))])
    low = [3 * f.mask] * (f.NL - 1)
    top = (4 * p - 1 - lval(f, low + [0])) // f.unit
    out += [low + [top], low + [0], [0] * (f.NL - 1) + [(4 * p - 1) // f.unit]]
    assert all(lval(f, b) < 4 * p and all(w < (3 << f.L) for w in b) for b in out)
    return out


def case_lazy_sub_wide(pr, f):
    bs = wide_operands(f)
    As = [x for v in extremes(f)[:8] for x in (lifts(f, v)[0], lifts(f, v)[-1])]
    rng = pyref.Xoshiro(21 + f.idx)
    pairs = [(a, b) for a in As for b in sample(bs, 400, 3)] + [(As[rng.next() % len(As)], b) for b in bs]
    got = pr.run(f, OP_F29_SUB_WIDE, [limbs(f, a) + b for a, b in pairs], f.NL, k=4)
    for (a, b), g in zip(pairs, got):
        assert_normalized(f, g, "f29_sub_wide<4,4>")
        assert lval(f, g) == a - lval(f, b) + 4 * f.p, (f, "f29_sub_wide<4,4>", hex(a), b)


def case_lazy_mul(pr, f):
    p, Rp = f.p, f.Rp
    Rpi = pow(Rp, -1, p)
    pairs = lazy_pairs(f)
    got = pr.run(f, OP_F29_MUL, [limbs(f, a) + limbs(f, b) for a, b in pairs], f.NL)
    for (a, b), g in zip(pairs, got):
        v = lval(f, g)
        assert_normalized(f, g, "f29_mul")
        assert v % p == a * b * Rpi % p and v < a * b // Rp + p + 1, (f, "f29_mul", hex(a), hex(b), hex(v))
    sq = [x for v in canon(f) for x in lifts(f, v)]
    got = pr.run(f, OP_F29_SQR, [limbs(f, a) for a in sq], f.NL)
    for a, g in zip(sq, got):
        v = lval(f, g)
        assert_normalized(f, g, "f29_sqr")
        assert v % p == a * a * Rpi % p and v < a * a // Rp + p + 1, (f, "f29_sqr", hex(a), hex(v))


def case_lazy_mul_sub(pr, f):
    """a*b - c*d with one reduction; the multiplicands b and d also as the RAW outputs of f29_sub_raw / f29_add_raw, as the mixed
    addition passes them (limbs below 3*2^L)"""
    p, Rp = f.p, f.Rp
    Rpi = pow(Rp, -1, p)
    for K in ((8, FP2Z_K) if f.has_fp2 else (8,)):
        ex = extremes(f)
        hi = lambda v: lifts(f, v)[-1]
        cmax = lambda v: v + (K - 1) * p                     # c < K*p
        quads = []
        for a in ex[:10]:
            for c in ex[:10]:
                quads += [(limbs(f, a), limbs(f, hi(c)), limbs(f, cmax(c)), limbs(f, hi(a))),
                          (limbs(f, hi(a)), limbs(f, hi(c)), limbs(f, c), limbs(f, a)),
                          (limbs(f, hi(a)), limbs(f, hi(a)), limbs(f, cmax(c)), limbs(f, hi(c)))]
        # raw multiplicands, formed here: b = x - y + 8p limb-wise without the carry sweep (what case_lazy_sub pins f29_sub_raw<8>
        # to), d = x + y + y limb-wise
        sp = [(hi(x), y + k * p) for x in ex[:10] for y in ex[:10] for k in (0, 6)]
        kp8 = kp_lend_limbs(f, 8)
        for x, y in sp:
            rb = [u + k - w for u, k, w in zip(limbs(f, x), kp8, limbs(f, y))]
            assert all(0 <= w < (3 << f.L) for w in rb[:-1]) and 0 <= rb[-1] < (1 << 31)
            rd = [u + 2 * w for u, w in zip(limbs(f, x), limbs(f, y))]
            quads.append((limbs(f, hi(y % p)), rb, limbs(f, cmax(x % p)), rd))
        rng = pyref.Xoshiro(31 + f.idx + K)
        cn = canon(f)
        pick = lambda: cn[rng.next() % len(cn)]
        def lifted():
            lf = lifts(f, pick())
            return limbs(f, lf[rng.next() % len(lf)])
        for _ in range(2000):
            quads.append((lifted(), lifted(), limbs(f, pick() + (rng.next() % K) * p), lifted()))
        got = pr.run(f, OP_F29_MUL_SUB, [a + b + c + d for a, b, c, d in quads], f.NL, k=K)
        for (a, b, c, d), g in zip(quads, got):
            a, b, c, d = (lval(f, x) for x in (a, b, c, d))
            v = lval(f, g)
            assert_normalized(f, g, "f29_mul_sub<%d>" % K)
            assert v % p == (a * b - c * d) * Rpi % p, (f, K, "f29_mul_sub", hex(a), hex(b), hex(c), hex(d), hex(v))
            assert v < (a * b + (K * p - c) * d) // Rp + p + 1 <= (a * b + K * p * d) // Rp + p + 1, (f, K, "f29_mul_sub bound", hex(v))


def reduce_3p_quotient(f, v):
    """the quotient estimate of f29_reduce_3p, from its definition: q = ((v >> (BITS-4)) * MU12) >> 12, MU12 = floor(2^(BITS+8) / p)"""
    return ((v >> (f.bits - 4)) * ((1 << (f.bits + 8)) // f.p)) >> 12


def reduce_3p_bound(f, below=None):
    """The largest residue f29_reduce_3p can leave, from its definition alone: q = ((v >> (BITS-4)) * MU12) >> 12 with
    MU12 = floor(2^(BITS+8) / p) (constants.h), so for the top-limb estimate t = v >> (BITS-4) the residue is at most
    (t+1)*2^(BITS-4) - 1 - q(t)*p.  Maximised over every t a normalized v < below (default: 2^(NL*L)) can have; below is a multiple of
    2^(BITS-4).  Returns (bound, max quotient deficit)."""
    mu = (1 << (f.bits + 8)) // f.p
    sh = f.bits - 4
    below = f.Rp if below is None else below
    assert below % (1 << sh) == 0
    worst, deficit = 0, 0
    for t in range(below >> sh):
        q = (t * mu) >> 12
        hi = ((t + 1) << sh) - 1
        assert q * f.p <= (t << sh), "the estimate is too large"
        worst = max(worst, hi - q * f.p)
        deficit = max(deficit, hi // f.p - q)
    return worst + 1, deficit


@functools.lru_cache(maxsize=None)
def hat_limit(f):
    """The largest V <= R' such that f29_reduce_3p leaves every normalized v < V below 3p and within the 32N-bit words -- the
    precondition of its consumers f29_is_zero_mod_p (candidates 0, p, 2p), f29_pack_canonical (two conditional subtractions) and
    f29_pack_hat.  By the enumeration of reduce_3p_bound: the first top-limb estimate t whose largest residue leaves that range ends it.
    R' for every field but BLS12-377 Fp, whose MU12 = 304 stands for 304.7."""
    mu = (1 << (f.bits + 8)) // f.p
    sh = f.bits - 4
    for t in range(f.Rp >> sh):
        if ((t + 1) << sh) - 1 - ((t * mu) >> 12) * f.p >= min(3 * f.p, f.R):
            return t << sh
    return f.Rp


# how far the exhaustive part of the operand set reaches where R' / p is too large for all of it (BLS12-377 Fp: 38996), and the size
# of the seeded samples above it
REDUCTION_DENSE_LOG2, REDUCTION_SAMPLE = 388, 1000


@functools.lru_cache(maxsize=None)
def reduction_operands(f):
    """k*p - 1, k*p, k*p + 1 for EVERY k that fits R', t*2^(BITS-4) - 1 and t*2^(BITS-4) for every top-limb estimate t, and the lifts
    of the canonical set up to R'.  BLS12-377 Fp (R' / p = 38996, 2^19 estimates): every k and every t below 2^388 -- which covers
    hat_limit and the range every consumer lives in -- and above it a seeded sample of both up to R'.  Every field with a hat_limit
    below R' also gets the values around it: the last estimate that is good, the first that is not and its largest value."""
    p, sh = f.p, f.bits - 4
    nk, nt = f.Rp // p + 1, (f.Rp >> sh) + 1
    ks, ts = range(nk), range(nt)
    if 3 * nk + 2 * nt > 80000:
        dense = 1 << REDUCTION_DENSE_LOG2
        assert hat_limit(f) + (1 << sh) < dense < f.Rp
        rng = pyref.Xoshiro(0x3E0 + f.idx)
        dk, dt = dense // p + 1, (dense >> sh) + 1
        ks = list(range(dk)) + sorted({dk + rng.next() % (nk - dk) for _ in range(REDUCTION_SAMPLE)}) + [nk - 1]
        ts = list(range(dt)) + sorted({dt + rng.next() % (nt - dt) for _ in range(REDUCTION_SAMPLE)}) + [nt - 2, nt - 1]
    vs = [x for k in ks for x in (k * p - 1, k * p, k * p + 1)]
    vs += [x for t in ts for x in ((t << sh) - 1, t << sh)]
    vs += [x for v in canon(f) for x in lifts(f, v) + [lifts(f, v, limit=f.Rp)[-1]]]
    hl = hat_limit(f)
    if hl < f.Rp:
        vs += [hl - (1 << sh), hl - 1, hl, hl + (1 << sh) - 1] + [x for v in canon(f)[:64] for x in lifts(f, v, limit=hl)[-1:]]
    vs = [v for v in dict.fromkeys(vs) if 0 <= v < f.Rp]
    assert len(vs) < 80000, (f, len(vs))
    return tuple(vs)


def case_lazy_reductions(pr, f):
    p = f.p
    vs = reduction_operands(f)
    hl = hat_limit(f)
    bound, deficit = reduce_3p_bound(f, hl)
    # what the consumers of f29_reduce_3p need: the three candidates 0, p, 2p of f29_is_zero_mod_p and the two conditional subtractions
    # of f29_pack_canonical cover [0, 3p), and the residue must fit the 32N-bit words
    assert bound <= 3 * p and bound <= f.R and deficit <= 2, (f, bound / p, deficit)
    # where that holds, from the definition: for any normalized value but on BLS12-377 Fp, where lazy_bounds.check_reduce_3p finds the
    # same first value that leaves it -- above 2^386.5 as field29.hip.h says, below the 2^390 the lazy representation allows
    fb = lazy_bounds.check_reduce_3p(p, f.L, f.NL)[1]
    if f.name == "bls12_377_fp":
        assert fb == math.log2(hl) and (1 << 773) < hl * hl and hl < f.Rp // 4, (f, math.log2(hl), fb)
    else:
        assert hl == f.Rp and (fb is None or 2 ** fb >= f.Rp), (f, hl.bit_length(), fb)
    if f.name == "bls12_377_fr":
        # ... and what the definition gives for this modulus (MU12 = 438 stands for 438.8): at most 1 short, the residue below 1.87 r
        assert deficit <= 1 and 100 * bound < 187 * p, (f, bound / p, deficit)
    elif f.name != "bls12_377_fp":
        # ... and what the definition gives for these four moduli: the estimate is at most 1 short, the residue below 1.35 p
        assert deficit <= 1 and 100 * bound < 135 * p, (f, bound / p, deficit)
    if f.is_base:
        # every coordinate the point formulas can hold (the exact fixed points of the interval analysis) is below hat_limit: what
        # f29_is_zero_mod_p and f29_pack_hat are given in the kernels is inside their precondition
        for fp2 in ((False, True) if f.has_fp2 else (False,)):
            for fn in (lazy_bounds.check, lazy_bounds.check_add, lazy_bounds.check_dbl, lazy_bounds.check_mdbl, lazy_bounds.check_ladder):
                B = exact_bounds(fn, f, fp2)
                assert set(B) == {"X", "Y", "ZZ", "ZZZ"} and all(v < hl for v in B.values()), (f, fn.__name__, fp2, B)
    for lo in range(0, len(vs), 30000):
        chunk = vs[lo:lo + 30000]
        rows = [limbs(f, v) for v in chunk]
        r3 = pr.run(f, OP_F29_REDUCE_3P, rows, f.NL)
        prd = pr.run(f, OP_F29_PARTIAL_REDUCE, rows, f.NL)
        zz = pr.run(f, OP_F29_IS_ZERO_MOD_P, rows, 1)
        ph = pr.run(f, OP_F29_PACK_HAT, rows, f.N)
        # f29_pack_canonical after the step, on the step's own output where that is inside its precondition (below: checked exactly)
        ok = [i for i, v in enumerate(chunk) if v < hl]
        pc = dict(zip(ok, pr.run(f, OP_F29_PACK_CANONICAL, [r3[i] for i in ok], f.N)))
        for i, (v, g, h, z, c) in enumerate(zip(chunk, r3, prd, zz, ph)):
            assert_normalized(f, g, "f29_reduce_3p")
            r = lval(f, g)
            # the exact pin, for ANY normalized value: v - q*p with the q of the definition
            assert r == v - reduce_3p_quotient(f, v) * p, (f, "f29_reduce_3p", hex(v), hex(r), r / p)
            assert_normalized(f, h, "f29_partial_reduce")
            rr = lval(f, h)
            q = v >> f.bits
            assert rr == v - q * p and rr < (1 << f.bits) + q * ((1 << f.bits) - p), (f, "f29_partial_reduce", hex(v), hex(rr))
            # below 4p for v < 2^(BITS+3) needs 2^BITS + 7 (2^BITS - p) <= 4p, a modulus above 8/11 * 2^BITS: every field but BLS12-377's
            # Fr (0.58 * 2^BITS; field29.hip.h: no caller of f29_partial_reduce is built over it), which keeps the bound above alone
            assert 11 * p >= (8 << f.bits) or f.name == "bls12_377_fr"
            assert v >= (1 << (f.bits + 3)) or rr < 4 * p or 11 * p < (8 << f.bits), (f, "f29_partial_reduce: not below 4p", hex(v))
            if v < hl:
                assert r % p == v % p and r <= v and r < bound, (f, "f29_reduce_3p", hex(v), hex(r), r / p)
                assert z[0] == (1 if v % p == 0 else 0), (f, "f29_is_zero_mod_p", hex(v), z)
                assert wval(pc[i]) == v % p, (f, "f29_pack_canonical after f29_reduce_3p", hex(v), hex(wval(pc[i])))
                assert wval(c) == v % p, (f, "f29_pack_hat", hex(v), hex(wval(c)))


def case_lazy_inv(pr, f):
    p, Rp = f.p, f.Rp
    vs = [x for v in extremes(f) for x in lifts(f, v)] + sample([x for v in canon(f) for x in lifts(f, v)], 150, 41)
    got = pr.run(f, OP_F29_INV, [limbs(f, v) for v in vs], f.NL)
    for v, g in zip(vs, got):
        r = lval(f, g)
        assert_normalized(f, g, "f29_inv")
        assert r % p == pow(v, p - 2, p) * Rp * Rp % p and r < 2 * p, (f, "f29_inv", hex(v), hex(r))


# ---- Fp2 ------------------------------------------------------------------------------------------------------------------------
def fp2_operands(f, kmax, n, seed):
    """pairs (c0, c1) of lifted values below kmax*p"""
    ex = extremes(f)
    corner = lambda v: v + (kmax - 1) * f.p
    out = [(a, b) for a in ex[:8] for b in ex[:8]] + [(corner(a), corner(b)) for a in ex[:8] for b in ex[:8]]
    out += [(a, corner(b)) for a in ex[:8] for b in ex[:8]] + [(corner(a), b) for a in ex[:8] for b in ex[:8]]
    rng = pyref.Xoshiro(seed + f.idx)
    cn = canon(f)
    out += [(cn[rng.next() % len(cn)] + (rng.next() % kmax) * f.p, cn[rng.next() % len(cn)] + (rng.next() % kmax) * f.p) for _ in range(n)]
    return out


def l2(f, a):
    return limbs(f, a[0]) + limbs(f, a[1])


def v2(f, row):
    return lval(f, row[:f.NL]), lval(f, row[f.NL:])


def case_fp2(pr, f):
    p, Rp, K = f.p, f.Rp, FP2Z_K
    Rpi = pow(Rp, -1, p)
    F = pyref.Fp2Ops(p)
    scale = lambda z: (z[0] * Rpi % p, z[1] * Rpi % p)
    red = lambda z: (z[0] % p, z[1] % p)
    A = fp2_operands(f, K, 300, 51)
    B = fp2_operands(f, K, 300, 52)
    rng = pyref.Xoshiro(53 + f.idx)
    pairs = [(A[rng.next() % len(A)], B[rng.next() % len(B)]) for _ in range(3000)] + list(zip(A, B))
    got = pr.run(f, OP_F29X2_MUL, [l2(f, a) + l2(f, b) for a, b in pairs], 2 * f.NL)
    for (a, b), g in zip(pairs, got):
        assert_normalized(f, g[:f.NL], "Fp2 f29_mul c0"), assert_normalized(f, g[f.NL:], "Fp2 f29_mul c1")
        r = v2(f, g)
        assert red(r) == scale(F.mul(red(a), red(b))), (f, "Fp2 f29_mul", a, b, r)
        assert r[0] < (a[0] * b[0] + (K * p - a[1]) * b[1]) // Rp + p + 1 and r[1] < (a[0] * b[1] + a[1] * b[0]) // Rp + p + 1, (f, "Fp2 f29_mul bound")
    S = fp2_operands(f, 8, 600, 54)                          # the square subtracts with 8p
    got = pr.run(f, OP_F29X2_SQR, [l2(f, a) for a in S], 2 * f.NL)
    for a, g in zip(S, got):
        assert_normalized(f, g[:f.NL], "Fp2 f29_sqr c0"), assert_normalized(f, g[f.NL:], "Fp2 f29_sqr c1")
        r = v2(f, g)
        assert red(r) == scale(F.mul(red(a), red(a))), (f, "Fp2 f29_sqr", a, r)
        assert r[0] < (a[0] + a[1]) * (a[0] - a[1] + 8 * p) // Rp + p + 1 and r[1] < 2 * (a[0] * a[1] // Rp + p) + 1, (f, "Fp2 f29_sqr bound")
    quads = [(A[rng.next() % len(A)], B[rng.next() % len(B)], A[rng.next() % len(A)], B[rng.next() % len(B)]) for _ in range(3000)]
    quads += [(A[i], B[i], A[-1 - i], B[-1 - i]) for i in range(256)]
    got = pr.run(f, OP_F29X2_MUL_SUB, [l2(f, a) + l2(f, b) + l2(f, c) + l2(f, d) for a, b, c, d in quads], 2 * f.NL, k=K)
    Kp = K * p
    for (a, b, c, d), g in zip(quads, got):
        assert_normalized(f, g[:f.NL], "Fp2 f29_mul_sub c0"), assert_normalized(f, g[f.NL:], "Fp2 f29_mul_sub c1")
        r = v2(f, g)
        assert red(r) == scale(F.sub(F.mul(red(a), red(b)), F.mul(red(c), red(d)))), (f, "Fp2 f29_mul_sub", a, b, c, d, r)
        re = a[0] * b[0] + (Kp - a[1]) * b[1] + (Kp - c[0]) * d[0] + c[1] * d[1]
        im = a[0] * b[1] + a[1] * b[0] + (Kp - c[0]) * d[1] + (Kp - c[1]) * d[0]
        assert r[0] < re // Rp + p + 1 and r[1] < im // Rp + p + 1, (f, "Fp2 f29_mul_sub bound")
    I = fp2_operands(f, 4, 60, 55)
    got = pr.run(f, OP_F29X2_INV, [l2(f, a) for a in I], 2 * f.NL)
    for a, g in zip(I, got):
        r = v2(f, g)
        want = (0, 0) if red(a) == (0, 0) else F.inv(red(a))
        assert red(r) == (want[0] * Rp * Rp % p, want[1] * Rp * Rp % p) and r[0] < 2 * p and r[1] <= 2 * p, (f, "Fp2 f29_inv", a, r)


# ---- point formulas at the top of their intervals -----------------------------------------------------------------------------------
class PointCtx:
    """the group, the field operations and the coordinate codec of one (curve, group)"""

    def __init__(self, f, fp2):
        self.f, self.fp2 = f, fp2
        self.c = CURVE_BY_NAME[f.curve]
        assert f.has_fp2 or not fp2
        self.G = pyref.g2_group(self.c) if fp2 else pyref.g1_group(self.c)
        self.F = self.G.F
        self.gen = self.c.g2 if fp2 else self.c.g1
        self.nw = (2 if fp2 else 1) * f.NL
        self.op = OP_PT2 if fp2 else 0

    def comps(self, c):
        return tuple(c) if self.fp2 else (c,)

    def elem(self, comps):
        return tuple(x % self.f.p for x in comps) if self.fp2 else comps[0] % self.f.p

    def enc(self, c, bound):
        """a field element as lazy limbs: the hat-domain value of each component, lifted to the largest multiple-of-p offset below bound"""
        f, out = self.f, []
        for x in self.comps(c):
            h = x * f.Rp % f.p
            out += limbs(f, h + (bound - 1 - h) // f.p * f.p if bound > f.p else h)
        return out

    def enc_neg_y(self, y):
        """the negated y of a table point as the kernels form it: 2p - hat(y) per component"""
        f, out = self.f, []
        for x in self.comps(y):
            out += limbs(f, 2 * f.p - x * f.Rp % f.p)
        return out

    def dec(self, row):
        f = self.f
        return tuple(lval(f, row[i * f.NL:(i + 1) * f.NL]) for i in range(2 if self.fp2 else 1))

    def xyzz(self, P, lam):
        """a valid XYZZ representation of the affine P with ZZ = lam^2 (lam = one: ZZ = ZZZ = 1)"""
        F = self.F
        zz = F.mul(lam, lam)
        zzz = F.mul(zz, lam)
        return (F.mul(P[0], zz), F.mul(P[1], zzz), zz, zzz)

    def enc_pt(self, Q, bounds):
        return [w for c, k in zip(Q, ("X", "Y", "ZZ", "ZZZ")) for w in self.enc(c, bounds[k])]

    def dec_pt(self, row, bounds, what):
        """the four coordinates as raw integers (per component), each checked against its bound"""
        out = []
        for i, k in enumerate(("X", "Y", "ZZ", "ZZZ")):
            seg = row[i * self.nw:(i + 1) * self.nw]
            for j in range(self.nw // self.f.NL):
                assert_normalized(self.f, seg[j * self.f.NL:(j + 1) * self.f.NL], what)
            v = self.dec(seg)
            assert all(x < bounds[k] for x in v), (what, "coordinate", k, "leaves the bound of the interval analysis", [x / bounds[k] for x in v])
            out.append(v)
        return out

    def affine(self, coords):
        """raw XYZZ coordinates (hat domain, unreduced) -> affine point; None when ZZ = 0 (mod p)"""
        F = self.F
        X, Y, ZZ, ZZZ = (self.elem(c) for c in coords)
        if F.is_zero(ZZ) or F.is_zero(ZZZ):
            return None
        return (F.mul(X, F.inv(ZZ)), F.mul(Y, F.inv(ZZZ)))   # the factor R' of the hat domain cancels

    def points(self):
        """the generator and multiples by seeded full-size scalars: no two are related by a small factor, so a chain of 50 additions
        of one to another never meets an exceptional case by accident"""
        rng = pyref.Xoshiro(0x9017 + self.f.idx)
        return [self.gen] + [self.G.mul(self.gen, rng.field(self.c.r)) for _ in range(5)]

    def lams(self):
        p = self.f.p
        if self.fp2:
            return [(1, 0), (p - 1, p - 1), (0x1234567, 0x7654321), ((p - 1) // 2, 2)]
        return [1, p - 1, 0x1234567, (p - 1) // 2]


def _zero_detected(pr, f, comps):
    """f29_is_zero_mod_p on each component of a coordinate"""
    return all(z[0] == 1 for z in pr.run(f, OP_F29_IS_ZERO_MOD_P, [limbs(f, x) for x in comps], 1))


def exact_bounds(fn, f, fp2, **kw):
    return fn(f.curve, fp2, exact=True, **kw)


def case_point_add29(pr, f, fp2):
    C = PointCtx(f, fp2)
    B = exact_bounds(lazy_bounds.check_add, f, fp2)
    P, lam = C.points(), C.lams()
    cases = [(P[i], lam[i % 4], P[j], lam[(i + j) % 4]) for i in range(len(P)) for j in range(len(P)) if i != j]
    rows = [C.enc_pt(C.xyzz(a, la), B) + C.enc_pt(C.xyzz(b, lb), B) for a, la, b, lb in cases]
    for k in (1, 50):
        got = pr.run(f, OP_PT_ADD29 + C.op, rows, 4 * C.nw, k=k)
        for (a, la, b, lb), g in zip(cases, got):
            assert C.affine(C.dec_pt(g, B, "add29 x%d" % k)) == C.G.add(a, C.G.mul(b, k)), (f, fp2, "add29", k)
    # exceptional: the same point, the opposite point (in different representations), an operand at infinity -> ZZ = 0 (mod p),
    # found by f29_is_zero_mod_p, and it stays there
    inf = (C.F.one, C.F.one, C.F.zero, C.F.zero)
    exc = [(C.xyzz(P[2], lam[1]), C.xyzz(P[2], lam[2])), (C.xyzz(P[2], lam[0]), C.xyzz(C.G.neg(P[2]), lam[3])),
           (inf, C.xyzz(P[1], lam[2])), (C.xyzz(P[1], lam[2]), inf)]
    rows = [C.enc_pt(a, B) + C.enc_pt(b, B) for a, b in exc]
    for k in (1, 50):
        for g in pr.run(f, OP_PT_ADD29 + C.op, rows, 4 * C.nw, k=k):
            co = C.dec_pt(g, B, "add29 exceptional")
            assert C.affine(co) is None and _zero_detected(pr, f, co[2]), (f, fp2, "add29: exceptional input not flagged by ZZ")


def case_point_dbl29(pr, f, fp2):
    C = PointCtx(f, fp2)
    B = exact_bounds(lazy_bounds.check_dbl, f, fp2)
    cases = [(a, la) for a in C.points() for la in C.lams()[:3]]
    rows = [C.enc_pt(C.xyzz(a, la), B) for a, la in cases]
    for k in (1, 50):
        got = pr.run(f, OP_PT_DBL29 + C.op, rows, 4 * C.nw, k=k)
        for (a, la), g in zip(cases, got):
            assert C.affine(C.dec_pt(g, B, "dbl29 x%d" % k)) == C.G.mul(a, 1 << k), (f, fp2, "dbl29", k)


def case_point_madd29(pr, f, fp2):
    C = PointCtx(f, fp2)
    B = exact_bounds(lazy_bounds.check, f, fp2)
    P, lam = C.points(), C.lams()
    cases = [(P[i], lam[(i + j) % 4], P[j], neg) for i in range(len(P)) for j in range(len(P)) if i != j
             for neg in (False, True)]
    def row(a, la, q, neg):
        return C.enc_pt(C.xyzz(a, la), B) + C.enc(q[0], 0) + (C.enc_neg_y(q[1]) if neg else C.enc(q[1], 0))
    rows = [row(*c) for c in cases]
    for k in (1, 50):
        got = pr.run(f, OP_PT_MADD29 + C.op, rows, 4 * C.nw, k=k)
        gotc = pr.run(f, OP_PT_MADD29_COMPLETE + C.op, rows, 4 * C.nw + 1, k=k)
        for (a, la, q, neg), g, gc in zip(cases, got, gotc):
            want = C.G.add(a, C.G.mul(C.G.neg(q) if neg else q, k))
            assert C.affine(C.dec_pt(g, B, "madd29 x%d" % k)) == want, (f, fp2, "madd29", k, neg)
            assert gc[-1] == 1 and gc[:-1] == g, (f, fp2, "madd29_complete differs from madd29 on an ordinary addition", k)
    # exceptional inputs through the fast loop: ZZ = 0 (mod p) and detected
    inf = (C.F.one, C.F.one, C.F.zero, C.F.zero)
    exc = [(C.xyzz(P[2], lam[1]), P[2], False), (C.xyzz(P[2], lam[2]), P[2], True), (C.xyzz(C.G.neg(P[4]), lam[3]), P[4], False),
           (inf, P[1], False)]
    rows = [C.enc_pt(a, B) + C.enc(q[0], 0) + (C.enc_neg_y(q[1]) if neg else C.enc(q[1], 0)) for a, q, neg in exc]
    for k in (1, 50):
        for g in pr.run(f, OP_PT_MADD29 + C.op, rows, 4 * C.nw, k=k):
            co = C.dec_pt(g, B, "madd29 exceptional")
            assert C.affine(co) is None and _zero_detected(pr, f, co[2]), (f, fp2, "madd29: exceptional input not flagged by ZZ")


def case_point_mdbl29(pr, f, fp2):
    C = PointCtx(f, fp2)
    B = exact_bounds(lazy_bounds.check_mdbl, f, fp2)
    cases = [(q, neg) for q in C.points() for neg in (False, True)]
    rows = [C.enc(q[0], 0) + (C.enc_neg_y(q[1]) if neg else C.enc(q[1], 0)) for q, neg in cases]
    got = pr.run(f, OP_PT_MDBL29 + C.op, rows, 4 * C.nw, k=1)
    for (q, neg), g in zip(cases, got):
        assert C.affine(C.dec_pt(g, B, "mdbl29")) == C.G.mul(C.G.neg(q) if neg else q, 2), (f, fp2, "mdbl29", neg)


def case_point_madd29_complete(pr, f, fp2):
    """the same point -> the doubling; the opposite point -> false; the accumulator at the top of the bounds the mixed additions
    reach when they start from a doubling's output (lazy_bounds.check with init = check_mdbl)"""
    C = PointCtx(f, fp2)
    D = exact_bounds(lazy_bounds.check_mdbl, f, fp2)
    B = exact_bounds(lazy_bounds.check, f, fp2, init=(D["X"], D["Y"], D["ZZ"], D["ZZZ"]))
    P, lam = C.points(), C.lams()
    qy = lambda q, neg: C.enc_neg_y(q[1]) if neg else C.enc(q[1], 0)
    same = [(C.xyzz(C.G.neg(q) if neg else q, la), q, neg) for q in P[:4] for la in lam for neg in (False, True)]
    opp = [(C.xyzz(q if neg else C.G.neg(q), la), q, neg) for q in P[:4] for la in lam for neg in (False, True)]
    rows = [C.enc_pt(a, B) + C.enc(q[0], 0) + qy(q, neg) for a, q, neg in same + opp]
    got = pr.run(f, OP_PT_MADD29_COMPLETE + C.op, rows, 4 * C.nw + 1, k=1)
    # P = f29_mul(X2, ZZ1) - X1 + K*p is a NONZERO multiple of p as an integer for every one of these: it is 0 (mod p) since the
    # points agree in x, and the product is a non-negative integer while the lifted X1 stays below K*p, component by component
    K = 4 if fp2 else 8
    for a, q, neg in same:
        x1 = C.dec(C.enc(a[0], B["X"]))
        assert all(x < K * f.p for x in x1), (f, fp2, "the lifted X1 does not make P a nonzero multiple of p")
    for (a, q, neg), g in zip(same, got[:len(same)]):
        assert g[-1] == 1, (f, fp2, "madd29_complete: the same point was not doubled")
        assert C.affine(C.dec_pt(g[:-1], D, "madd29_complete doubling")) == C.G.mul(C.G.neg(q) if neg else q, 2), (f, fp2, "madd29_complete doubling")
    for (a, q, neg), g in zip(opp, got[len(same):]):
        assert g[-1] == 0, (f, fp2, "madd29_complete: P + (-P) not reported")


POINT_CASES = {"add29": case_point_add29, "dbl29": case_point_dbl29, "madd29": case_point_madd29, "mdbl29": case_point_mdbl29,
               "madd29_complete": case_point_madd29_complete}

FIELD_CASES = {
    "packed_binary": case_packed_binary, "packed_unary": case_packed_unary, "conversions": case_conversions,
    "lazy_add_normalize": case_lazy_add_normalize, "lazy_sub": case_lazy_sub, "lazy_sub_wide": case_lazy_sub_wide,
    "lazy_mul": case_lazy_mul, "lazy_mul_sub": case_lazy_mul_sub, "lazy_reductions": case_lazy_reductions, "lazy_inv": case_lazy_inv,
}
BASE_FIELD_CASES = {"fp2": case_fp2}


# ---- boundary inputs through the shipped library (ctx: the emulation's or the device's context) ---------------------------------
def crafted_scalars(r, c):
    """scalars whose signed c-bit digits sit at the recoding's edges: every digit 2^(c-1) (the largest that stays positive),
    2^(c-1) + 1 (negative, and a carry through all windows into the top one), 2^c - 1; each as the largest such pattern below r
    and with fewer windows filled; and r - 1, r - 2, 2^(c-1), 1, 0"""
    bits = r.bit_length()
    nwin = bits // c + 1
    out = [r - 1, r - 2, 1 << (c - 1), (1 << (c - 1)) + 1, 1, 0]
    for d in ((1 << (c - 1)), (1 << (c - 1)) + 1, (1 << c) - 1):
        for m in sorted({1, 2, nwin - 2, nwin - 1, nwin}):
            low = sum(d << (c * w) for w in range(m)) & ((1 << (c * m)) - 1)
            if low < r:
                out.append(low)
            hi = (r >> (c * m)) << (c * m) | low             # the same low digits under r's own top bits
            out += [x for x in (hi, hi - (1 << (c * m))) if 0 <= x < r]
    return list(dict.fromkeys(out))


def sqrt_fp(a, p):
    """a square root of a mod p, or None: the exponentiation for p = 3 (mod 4); Tonelli-Shanks for BLS12-377's p (p - 1 = 2^46 * odd)"""
    a %= p
    if a == 0:
        return 0
    if pow(a, (p - 1) // 2, p) != 1:
        return None
    if p % 4 == 3:
        return pow(a, (p + 1) // 4, p)
    e, q = 0, p - 1
    while q % 2 == 0:
        e, q = e + 1, q // 2
    z = next(z for z in range(2, 1000) if pow(z, (p - 1) // 2, p) == p - 1)
    m, c, t, x = e, pow(z, q, p), pow(a, q, p), pow(a, (q + 1) // 2, p)
    while t != 1:
        i, u = 0, t
        while u != 1:
            i, u = i + 1, u * u % p
        b = pow(c, 1 << (m - i - 1), p)
        m, c, t, x = i, b * b % p, t * b * b % p, x * b % p
    return x


def crafted_bases(c):
    """G1 points whose Montgomery-image x carries the limb patterns of the operand set: x = pattern * R^-1, the pattern's lowest word
    stepped upward (at most 64 steps) until x^3 + b is a square; both signs of y.  On the two BLS12 curves these lie outside the
    r-torsion: the reference is pyref's curve arithmetic, never a discrete logarithm."""
    f = fp_of(c)
    p, Ri = f.p, pow(f.R, -1, f.p)
    pats = [1, 0xFFFFFFFF << 32, 0xFFFFFFFF << (32 * (f.N - 2)), f.mask << f.L, f.mask << (f.L * (f.NL - 2)), (1 << (f.bits - 1)) - 1 - 64,
            p - 1 - 64, 1 << (32 * (f.N - 1))]
    pts = []
    for pat in pats:
        for step in range(65):
            assert step < 64, ("no curve point within 64 steps of the pattern", hex(pat))
            x = (pat + step) % p * Ri % p
            y = sqrt_fp((x * x * x + c.b) % p, p)
            if y is not None and y * y % p == (x * x * x + c.b) % p:
                pts += [(x, y), (x, p - y)]
                break
    return pts


def case_msm_crafted(ctx, c, cbits, table, setenv):
    """G1 MSM over the crafted bases and the scalars crafted for window width cbits, Montgomery and canonical scalars; table: through a
    pinned table forced to that width (GA_TABLE_C), else the raw-bases call (whose planned width the caller passes)"""
    from gnark_amd import ecc
    from helpers import fr_to_arr, jac_to_affine_py, pts_to_arr
    G = pyref.g1_group(c)
    bases = crafted_bases(c)
    assert all(G.on_curve(P) for P in bases)
    sc = crafted_scalars(c.r, cbits)
    pts = [bases[i % len(bases)] for i in range(len(sc))]
    assert len(sc) <= 256
    want = G.msm(pts, sc)
    P = pts_to_arr(c, 0, pts)
    if table:
        setenv("GA_TABLE_C", str(cbits))
        t = ecc.PrecomputedBases(ctx, c.name, 0, P)
        try:
            assert t.info()["window_bits"] == cbits
            assert jac_to_affine_py(c, 0, t.MultiExp(fr_to_arr(c, sc))) == want, (c.name, cbits, "table, Montgomery scalars")
            assert jac_to_affine_py(c, 0, t.MultiExp(fr_to_arr(c, sc, mont=False), montgomery=False)) == want, (c.name, cbits, "table, canonical scalars")
        finally:
            t.free()
    else:
        assert ecc.plan(c.name, 0, len(sc), lib=ctx.lib)[0] == cbits
        assert jac_to_affine_py(c, 0, ecc.MultiExp(ctx, c.name, 0, P, fr_to_arr(c, sc))) == want, (c.name, cbits, "raw, Montgomery scalars")
        assert jac_to_affine_py(c, 0, ecc.MultiExp(ctx, c.name, 0, P, fr_to_arr(c, sc, mont=False), montgomery=False)) == want, (c.name, cbits, "raw, canonical scalars")


def case_fr_vector_ops(ctx, c):
    """ga_fr_vec_mul and ga_fr_batch_invert (zeros interleaved) over the canonical operand set, host and device pointers;
    ga_fr_linear_combination (1 and 16 terms) and ga_fr_poly_evaluate over it, host and device pointers as well"""
    from helpers import arr_to_fr, fr_to_arr
    f = fr_of(c)
    r = c.r
    vals = [v for v in canon(f)]
    a = vals
    b = vals[7:] + vals[:7]
    A, Bv = fr_to_arr(c, a), fr_to_arr(c, b)
    n = len(a)
    want_mul = [x * y % r for x, y in zip(a, b)]
    inv_in = [x for v in vals for x in (v, 0)]
    want_inv = [pow(x, r - 2, r) for x in inv_in]
    lib = ctx.lib
    for on_device in (0, 1):
        out = np.zeros_like(A)
        V = fr_to_arr(c, inv_in)
        if on_device:
            dA, dB, dO, dV = ctx.to_device(A), ctx.to_device(Bv), ctx.malloc(A.nbytes), ctx.to_device(V)
            try:
                lib.check(lib.ga_fr_vec_mul(ctx.handle, c.cid, dA.ptr, dB.ptr, n, dO.ptr, 1))
                lib.check(lib.ga_fr_batch_invert(ctx.handle, c.cid, dV.ptr, len(inv_in), 1))
                out, V = dO.to_host(A.shape), dV.to_host(V.shape)
            finally:
                for d in (dA, dB, dO, dV):
                    d.free()
        else:
            lib.check(lib.ga_fr_vec_mul(ctx.handle, c.cid, A.ctypes.data, Bv.ctypes.data, n, out.ctypes.data, 0))
            lib.check(lib.ga_fr_batch_invert(ctx.handle, c.cid, V.ctypes.data, len(inv_in), 0))
        assert arr_to_fr(c, out) == want_mul, (c.name, "ga_fr_vec_mul", on_device)
        assert arr_to_fr(c, V) == want_inv, (c.name, "ga_fr_batch_invert", on_device)
    # the two C entry points themselves, host pointers and device pointers (the scalars, the point and the value stay on the host)
    import ctypes as C
    ex = list(extremes(f))
    for on_device in (0, 1):
        for k in (1, 16):
            vs = [vals[j:] + vals[:j] for j in range(k)]
            sc = [ex[(3 + 5 * j) % len(ex)] for j in range(k)]
            want = [sum(s * v[i] for s, v in zip(sc, vs)) % r for i in range(n)]
            V, S, out = [fr_to_arr(c, v) for v in vs], fr_to_arr(c, sc), np.zeros_like(A)
            dev = [ctx.to_device(v) for v in V] + [ctx.malloc(A.nbytes)] if on_device else []
            try:
                ptrs = (C.c_void_p * k)(*([d.ptr for d in dev[:k]] if on_device else [v.ctypes.data for v in V]))
                lib.check(lib.ga_fr_linear_combination(ctx.handle, c.cid, n, k, ptrs, S.ctypes.data, dev[k].ptr if on_device else out.ctypes.data, on_device))
                if on_device:
                    out = dev[k].to_host(A.shape)
            finally:
                for d in dev:
                    d.free()
            assert arr_to_fr(c, out) == want, (c.name, "ga_fr_linear_combination", k, on_device)
        Pv = fr_to_arr(c, vals)
        dP = ctx.to_device(Pv) if on_device else None
        try:
            for z in (r - 1, 1, 0, ex[8], (r - 1) // 2):
                Z, val = fr_to_arr(c, [z]), np.zeros(4, dtype=np.uint64)
                lib.check(lib.ga_fr_poly_evaluate(ctx.handle, c.cid, dP.ptr if on_device else Pv.ctypes.data, n, Z.ctypes.data, val.ctypes.data, on_device))
                assert arr_to_fr(c, val.reshape(1, 4))[0] == pyref._poly_eval(vals, z, r), (c.name, "ga_fr_poly_evaluate", hex(z), on_device)
        finally:
            if dP is not None:
                dP.free()


def fft_boundary_input(r, n, name):
    return {"all r-1": lambda: [r - 1] * n, "all 1": lambda: [1] * n, "r-1 first": lambda: [r - 1] + [0] * (n - 1),
            "r-1 last": lambda: [0] * (n - 1) + [r - 1], "alternating": lambda: [0 if i % 2 == 0 else r - 1 for i in range(n)]}[name]()


FFT_INPUTS = ("all r-1", "all 1", "r-1 first", "r-1 last", "alternating")
# a curve the C oracle does not know compares with pyref.fft, 2.3 s per transform at 2^17: there the grid is two inputs and the four
# modes (DIF, forward), (DIT, inverse), each on and off the coset; computed once per session, whatever the knob set
FFT_2P17_PYREF_INPUTS = ("all r-1", "alternating")
FFT_2P17_PYREF_MODES = ((pyref.DIF, False), (pyref.DIT, True))


@functools.lru_cache(maxsize=None)
def pyref_fft_image(cname, logn, name, dec, coset, inv):
    """pyref.fft of a boundary input as the memory image the library returns"""
    from helpers import fr_to_arr
    c = CURVE_BY_NAME[cname]
    a = fr_to_arr(c, pyref.fft(c, fft_boundary_input(c.r, 1 << logn, name), dec, on_coset=coset, inverse=inv))
    a.setflags(write=False)
    return a


def case_fft_boundary_inputs(ctx, c, logn):
    """all r-1, all 1, a single r-1 first / last, alternating 0 / r-1 through every (inverse, decimation, coset) mode vs the C oracle;
    BLS12-377, which the oracle does not know, vs pyref.fft / pyref.compute_h (at 2^17 on the reduced grid above, without compute_h)"""
    import oracle
    from gnark_amd import fft
    from helpers import fr_to_arr
    n, r = 1 << logn, c.r
    by_oracle = c.name in pyref.CURVES
    reduced = not by_oracle and logn >= 17
    d = fft.Domain(ctx, c.name, n)
    try:
        for name in (FFT_2P17_PYREF_INPUTS if reduced else FFT_INPUTS):
            v = fft_boundary_input(r, n, name)
            row = {x: fr_to_arr(c, [x])[0] for x in set(v)}
            a = np.array([row[x] for x in v], dtype=np.uint64)
            for dec in (pyref.DIF, pyref.DIT):
                for coset in (False, True):
                    for inv in (False, True):
                        if reduced and (dec, inv) not in FFT_2P17_PYREF_MODES:
                            continue
                        want = oracle.fft(c.cid, a, 1 if inv else 0, dec, coset, nthreads=2) if by_oracle else \
                            pyref_fft_image(c.name, logn, name, dec, coset, inv)
                        got = (d.FFTInverse if inv else d.FFT)(a, dec, coset)
                        assert np.array_equal(got, want), (c.name, logn, name, dec, coset, inv)
        if logn >= 2 and not reduced:   # compute_h with A = B = r-1, C = A*B
            m = n - 1
            A = fr_to_arr(c, [r - 1] * m)
            Cc = fr_to_arr(c, [1] * m)
            want = oracle.compute_h(c.cid, A, A, Cc, d.Cardinality) if by_oracle else \
                fr_to_arr(c, pyref.compute_h(c, [r - 1] * m, [r - 1] * m, [1] * m, d.Cardinality))
            assert np.array_equal(d.compute_h(A, A, Cc), want), (c.name, logn, "compute_h")
    finally:
        d.close()


PLONK_BSB = 16   # PLONK_MAX_BSB: the most BSB22 gates check_plonk_constraints (tools/lazy_bounds.py) assumes


def case_plonk_constant_inputs(ctx, c, n):
    """the PLONK quotient with every input polynomial a constant from {r-1, 1, 0} (a constant evaluates to itself on every coset, so
    every evaluation the constraint kernel sees sits at the extreme), 16 BSB22 gates, blinding coefficients all 0 and all r-1,
    challenges all r-1 and seeded; given in canonical and in Lagrange form; the plain and the pinned call.  Reference:
    pyref.plonk_quotient (no gate cap).  The numerator need not vanish on the domain: computeNumerator + divideByZH is a formula."""
    from gnark_amd import fft, plonk
    from helpers import arr_to_fr, fr_to_arr
    r = c.r
    rng = pyref.Xoshiro(0x9107 + n)
    names = list(plonk.IDS) + [x for i in range(PLONK_BSB) for x in ("Qcp%d" % i, "Pi2%d" % i)]
    consts = [{k: v for k in names} for v in (r - 1, 1, 0)]
    consts.append({k: (r - 1, 1, 0)[j % 3] for j, k in enumerate(names)})              # mixed: r-1 against 1 against 0
    consts.append({k: (r - 1, r - 1, 1)[(j * 5) % 3] for j, k in enumerate(names)})
    row = {v: fr_to_arr(c, [v])[0] for v in (r - 1, 1, 0)}
    d0 = fft.Domain(ctx, c.name, n)
    d1 = fft.Domain(ctx, c.name, plonk.Rho(n) * n)
    try:
        for ci, cv in enumerate(consts):
            for blind in (0, r - 1):
                chal = [r - 1] * 3 if (ci + (blind != 0)) % 2 == 0 else [rng.field(r) for _ in range(3)]
                alpha, beta, gamma = chal
                bp = {"Bl": [blind] * 2, "Br": [blind] * 2, "Bo": [blind] * 2, "Bz": [blind] * 3}
                can = {k: [v] + [0] * (n - 1) for k, v in cv.items()}
                want = pyref.plonk_quotient(c, n, {k: can[k] for k in plonk.IDS}, [can["Qcp%d" % i] for i in range(PLONK_BSB)],
                                            [can["Pi2%d" % i] for i in range(PLONK_BSB)], bp, alpha, beta, gamma)
                kw = dict(bp={k: fr_to_arr(c, v) for k, v in bp.items()}, alpha=fr_to_arr(c, [alpha]), beta=fr_to_arr(c, [beta]),
                          gamma=fr_to_arr(c, [gamma]))
                for lagr in ((), tuple(names)):   # canonical: [v, 0, ..]; Lagrange: v everywhere
                    def arr(k):
                        a = np.zeros((n, 4), dtype=np.uint64)
                        a[:] = row[cv[k]] if lagr else 0
                        a[0] = row[cv[k]]
                        return a
                    polys = {k: arr(k) for k in plonk.IDS}
                    qc, pi = [arr("Qcp%d" % i) for i in range(PLONK_BSB)], [arr("Pi2%d" % i) for i in range(PLONK_BSB)]
                    what = (c.name, n, ci, hex(blind), "Lagrange" if lagr else "canonical")
                    got = plonk.ComputeQuotient(d0, d1, polys, qc, pi, lagrange=lagr, **kw)
                    assert arr_to_fr(c, got) == want, what + ("plain",)
                    ppk = plonk.ProvingKey(d0, d1, {k: polys[k] for k in plonk.FIXED_IDS}, qc,
                                           lagrange=[x for x in lagr if x in plonk.FIXED_IDS or x.startswith("Qcp")])
                    try:
                        got = ppk.ComputeQuotient({k: polys[k] for k in plonk.PROOF_IDS}, pi,
                                                  lagrange=[x for x in lagr if x in plonk.PROOF_IDS or x.startswith("Pi2")], **kw)
                        assert arr_to_fr(c, got) == want, what + ("pinned",)
                    finally:
                        ppk.close()
    finally:
        d0.close()
        d1.close()


def signed_digits(s, cbits, ref):
    """the (key, value) pairs of the raw-bases recoding of s < r, window by window; ref: the probe's row, whose value of a skipped pair
    is taken over (never read: a digit of 2^c - 1 plus a carry gives 0 with the sign set)"""
    half = 1 << (cbits - 1)
    carry, want = 0, []
    for w in range(DIGIT_WINDOWS):
        d = ((s >> (cbits * w)) & (2 * half - 1)) + carry
        carry = 1 if d > half else 0
        d -= carry << cbits
        want += [0xFFFFFFFF, ref[2 * w + 1]] if d == 0 else [w * half + abs(d) - 1, 0x80000000 if d < 0 else 0]
    assert carry == 0
    return want


def unreduced_scalars(r, sc):
    """canonical scalars at and above r, any 256-bit integer being allowed: k*r - 1, k*r, k*r + 1 for every k up to 2^256 // r (the
    count of conditional subtractions DigitWalk needs: 5, 2 and 13 for the three curves), 2^256 - 1, the largest multiple of r less
    one, and each of sc plus the largest multiple of r that keeps it below 2^256"""
    top = (1 << 256) // r
    out = [k * r + d for k in range(1, top + 1) for d in (-1, 0, 1)]
    out += [(1 << 256) - 1, (1 << 256) - 1 - (1 << 256) % r]
    out += [s + ((1 << 256) - 1 - s) // r * r for s in sc]
    assert all(r - 1 <= x < (1 << 256) for x in out) and max(x // r for x in out) == top
    return list(dict.fromkeys(out))


def case_digit_walk(pr, c, cbits):
    """DigitWalk (msm_sort.hip.h) on the crafted scalars, Montgomery and canonical: the recoding is pinned to signed digits in
    (-2^(c-1), 2^(c-1)] -- a digit of exactly 2^(c-1) stays POSITIVE and carries nothing.  (-2^(c-1) with a carry is the same scalar
    and gives the same MSM, so only this test tells the two apart.)  Raw-bases keys: window * 2^(c-1) + |digit| - 1, ~0 for digit 0;
    value: point index (0 here) | sign << 31.  Then canonical scalars that are NOT below r (unreduced_scalars): the digits are those
    of s mod r."""
    f = fr_of(c)
    r, half = c.r, 1 << (cbits - 1)
    sc = crafted_scalars(r, cbits)
    assert any((s >> (cbits * w)) & (2 * half - 1) == half for s in sc for w in range(4)), "no digit at 2^(c-1)"
    for mont in (1, 0):
        rows = [words(f, s * f.R % r if mont else s) + [mont] for s in sc]
        got = pr.run(f, OP_DIGIT_WALK, rows, 2 * DIGIT_WINDOWS, k=cbits)
        for s, g in zip(sc, got):
            assert g == signed_digits(s, cbits, g), (c.name, cbits, mont, hex(s))
    big = unreduced_scalars(r, sc)
    got = pr.run(f, OP_DIGIT_WALK, [words(f, s) + [0] for s in big], 2 * DIGIT_WINDOWS, k=cbits)
    for s, g in zip(big, got):
        assert g == signed_digits(s % r, cbits, g), (c.name, cbits, "canonical, not below r", hex(s), s // r)


# ---- what the two test modules share ---------------------------------------------------------------------------------------------
CURVES = [pyref.BN254, pyref.BLS12_381, BLS12_377]
# window widths forced on a pinned table (the raw call's planned width is found by planned_width); for BLS12-381's 255-bit Fr, 15 and
# 17 divide 255, so the top window holds nothing but the carry; 11 and 23 divide the 253 bits of BLS12-377's
TABLE_C = {"bn254": [4, 13, 16], "bls12-381": [5, 15, 17], "bls12-377": [4, 11, 23]}
TABLE_CASES = [(c, w) for c in CURVES for w in TABLE_C[c.name]]
DIGIT_CASES = TABLE_CASES + [(c, w) for w in (8, 22) for c in CURVES]
FFT_LOGN = [1, 2, 3, 6, 10, 12]
# the knob sets of test_fft_wave_local_rounds (device: default, no-direct, round3) and of its emulation twin (no-wave-local as well)
FFT_2P17_KNOBS = {"default": {}, "no-direct": {"GA_NTT_DIRECT": "0"}, "no-wave-local": {"GA_NTT_WAVE_LOCAL": "0"},
                  "round3": {"GA_NTT_WAVE_LOCAL": "0", "GA_NTT_DIRECT": "0"}}


def planned_width(ctx, c):
    """the window width ga_msm_plan gives a raw G1 MSM over the scalars crafted for that width: the scalar count depends on the width
    and the planned width on the count, so settle (case_msm_crafted checks the result)"""
    from gnark_amd import ecc
    n = len(crafted_scalars(c.r, 8))
    for _ in range(3):
        cbits = ecc.plan(c.name, 0, n, lib=ctx.lib)[0]
        n = len(crafted_scalars(c.r, cbits))
    return cbits

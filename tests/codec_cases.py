"""The point codec of the key and proof readers (gnark_amd/csrc/keyio.hip.h: point_decode / point_encode, on the host for header points,
proofs and ga_point_unmarshal, on the device for every key vector) and the staging loops of key I/O under GA_KEY_CHUNK.

Part 1 is a STRICT big-integer restatement of the decoding rule, written from the rule and independent of keyio.hip.h and of pyref's
decoders (which assert and have no verdicts); pyref serves for field and curve arithmetic only.  The rule:
  flags        BN254: the top two bits of byte 0 -- 00 raw, 01 infinity (in both modes), 10 / 11 compressed with the smaller / larger y.
               BLS12-381 (ZCash): bit 7 compressed, bit 6 infinity, bit 5 larger y; 0b001, 0b011 and 0b111 are malformed.
  coordinates  every one canonical (< p), in G2 A1 and A0 separately (the encoding is A1 | A0, big-endian).
  compressed   x^3 + b is a square; of the two roots the flag names the "larger": y > (p - 1) / 2, in Fp2 decided by A1 and by A0 only
               when A1 = 0.
  raw          y^2 = x^3 + b (stricter than an unchecked gnark read, on purpose).
  infinity     the flag bits and nothing else: every other bit zero over the whole encoded length; an all-zero raw point is infinity
               too (the one leniency).
  in a vector  stride and mode are the stream's; a finite point or an infinity with the other mode's flag is refused (BLS12-381: 0x40
               in a compressed vector, 0xC0 in a raw one); BN254's one infinity flag is valid in both.
  header points, proofs   a point's length follows its own flag; a BN254 infinity takes the stream's mode (compressed while that is
               unknown); the zero check of an infinity runs over exactly the bytes consumed.
Part 2 builds the encoding table, part 3 runs it through the host route and the device route, part 4 is the multi-pass cases.  Every
case is a function of a context: tests/test_codec.py runs them on the emulation, tests/test_codec_gpu.py on the device."""
import ctypes as C
import dataclasses
import functools
import os
import tempfile

import numpy as np
import pytest

import pyref
from gnark_amd import groth16, synth
from gnark_amd._lib import GnarkAmdError
from helpers import BLS12_381, BN254, arr_to_g1_affine, arr_to_g2_affine, gen_of, group_of, pts_to_arr

CURVES = [BN254, BLS12_381]
REJECT = ("reject",)
KNOBS = (None, 1, 63, 64, 65)   # GA_KEY_CHUNK: unset, one point per pass, and the 64-thread block of the codec kernels -1, +0, +1
FORMATS = {"compressed": groth16.KEY_FORMAT_COMPRESSED, "raw": groth16.KEY_FORMAT_RAW, "dump": groth16.KEY_FORMAT_DUMP}


# ---- 1. the strict reference ------------------------------------------------------------------------------------------------------------
def coord_bytes(c, group):
    return c.fp_bytes * (1 if group == 0 else 2)


def enc_len(c, group, compressed):
    return coord_bytes(c, group) * (1 if compressed else 2)


def flag_mask(c):
    return 0x3F if c is BN254 else 0x1F


def flags_of(c, b0):
    """(compressed, infinity, largest) of a first byte, None when malformed"""
    if c is BN254:
        m = b0 >> 6
        return (m >= 2, m == 1, m == 3)
    comp, inf, large = bool(b0 & 0x80), bool(b0 & 0x40), bool(b0 & 0x20)
    if (inf and large) or (large and not comp):
        return None
    return (comp, inf, large)


def curve_b(c, group):
    return c.b if group == 0 else c.b2


def rhs_of(c, group, x):
    F = group_of(c, group).F
    return F.add(F.mul(F.mul(x, x), x), curve_b(c, group))


def is_square_fp(a, p):
    return a % p == 0 or pow(a, (p - 1) // 2, p) == 1


def sqrt_fp(a, p):
    s = pow(a, (p + 1) // 4, p)   # p = 3 mod 4
    return s if s * s % p == a % p else None


def fp2_pow(F, a, e):
    out = (1, 0)
    while e:
        if e & 1:
            out = F.mul(out, a)
        a = F.mul(a, a)
        e >>= 1
    return out


def sqrt_fp2(a, p):
    """a square root in Fp[u]/(u^2 + 1), p = 3 mod 4, by exponentiation in Fp2 alone (Adj, Rodriguez-Henriquez 2012, algorithm 9) -- not
    the complex method of the library and of pyref; None when a is no square"""
    F = pyref.Fp2Ops(p)
    if a == (0, 0):
        return (0, 0)
    a1 = fp2_pow(F, a, (p - 3) // 4)
    x0 = F.mul(a1, a)
    alpha = F.mul(a1, x0)
    if F.mul((alpha[0], (-alpha[1]) % p), alpha) == (p - 1, 0):
        return None
    if alpha == (p - 1, 0):
        x = F.mul((0, 1), x0)
    else:
        x = F.mul(fp2_pow(F, ((1 + alpha[0]) % p, alpha[1]), (p - 1) // 2), x0)
    assert F.mul(x, x) == a
    return x


def is_largest(c, group, y):
    half = (c.p - 1) // 2
    if group == 0:
        return y > half
    return y[1] > half if y[1] != 0 else y[0] > half


def split_coord(c, group, b, mask):
    """one coordinate from its big-endian bytes (G2: A1 | A0), None when a part is not canonical"""
    n = c.fp_bytes
    first = int.from_bytes(bytes([b[0] & mask]) + bytes(b[1:n]), "big")
    if first >= c.p:
        return None
    if group == 0:
        return first
    a0 = int.from_bytes(bytes(b[n:2 * n]), "big")
    return None if a0 >= c.p else (a0, first)


def decode_point(c, group, b, compressed):
    """one point of a stream whose mode is `compressed`, from exactly enc_len bytes: REJECT or ("accept", P), P = None for infinity"""
    b = bytes(b)
    assert len(b) == enc_len(c, group, compressed)
    cb = coord_bytes(c, group)
    f = flags_of(c, b[0])
    if f is None:
        return REJECT
    comp, inf, large = f
    if inf:
        if c is not BN254 and comp != compressed:
            return REJECT
        return ("accept", None) if not (b[0] & flag_mask(c)) and not any(b[1:]) else REJECT
    if comp != compressed:
        return REJECT
    if not compressed and not any(b):
        return ("accept", None)
    F = group_of(c, group).F
    x = split_coord(c, group, b[:cb], flag_mask(c))
    if x is None:
        return REJECT
    rhs = rhs_of(c, group, x)
    if compressed:
        y = sqrt_fp(rhs, c.p) if group == 0 else sqrt_fp2(rhs, c.p)
        if y is None:
            return REJECT
        if is_largest(c, group, y) != large:
            y = F.neg(y)
        return ("accept", (x, y))
    y = split_coord(c, group, b[cb:], 0xFF)
    if y is None or F.mul(y, y) != rhs:
        return REJECT
    return ("accept", (x, y))


def decode_header(c, group, data, mode):
    """a header point or a point of a proof at the head of `data`; mode: the stream's, -1 unknown, 0 raw, 1 compressed.
    REJECT or ("accept", P, consumed, mode after it)"""
    data = bytes(data)
    if not data:
        return REJECT
    f = flags_of(c, data[0])
    if f is None:
        return REJECT
    comp, inf, _ = f
    if inf and c is BN254:
        comp = mode != 0
    if not inf and mode < 0:
        mode = 1 if comp else 0
    ln = enc_len(c, group, comp)
    if len(data) < ln:
        return REJECT
    v = decode_point(c, group, data[:ln], comp)
    return REJECT if v == REJECT else ("accept", v[1], ln, mode)


def decode_proof(c, data, max_commitments=64):
    """Proof.ReadFrom under the rule above: REJECT or ("accept", ar, bs, krs, [commitments], pok, consumed)"""
    mode, off, pts = -1, 0, []

    def point(group):
        nonlocal mode, off
        v = decode_header(c, group, data[off:], mode)
        if v == REJECT:
            return False
        pts.append(v[1])
        off, mode = off + v[2], v[3]
        return True

    if not (point(0) and point(1) and point(0)) or len(data) - off < 4:
        return REJECT
    n = int.from_bytes(data[off:off + 4], "big")
    off += 4
    if n > max_commitments:
        return REJECT
    for _ in range(n + 1):
        if not point(0):
            return REJECT
    return ("accept", pts[0], pts[1], pts[2], pts[3:3 + n], pts[3 + n], off)


def encode_point(c, group, P, compressed):
    """the one encoding of an affine pair (x, y) -- the curve equation plays no part -- or of infinity (None)"""
    ln, cb = enc_len(c, group, compressed), coord_bytes(c, group)
    if P is None:
        return bytes([0x40 if c is BN254 or not compressed else 0xC0]) + bytes(ln - 1)
    be = lambda v: v.to_bytes(c.fp_bytes, "big") if group == 0 else v[1].to_bytes(c.fp_bytes, "big") + v[0].to_bytes(c.fp_bytes, "big")
    x, y = P
    if not compressed:
        return be(x) + be(y)
    out = bytearray(be(x))
    assert len(out) == cb
    large = is_largest(c, group, y)
    out[0] |= (0xC0 if large else 0x80) if c is BN254 else (0xA0 if large else 0x80)
    return bytes(out)


# ---- 2. the encoding table --------------------------------------------------------------------------------------------------------------
# a case: (name, bytes of one stride of the stream, verdict BY CONSTRUCTION inside a vector: the point, None for infinity, or REJECT).
# The reference must agree with the construction (test_reference_agrees_with_construction) before it judges the library.
SEARCH_BOUND = 400   # draws of every seeded search below; the searches end far inside it (asserted where they run)


def _search(name, draw, good, bound=SEARCH_BOUND):
    for i in range(bound):
        v = draw(i)
        if good(v):
            return v
    raise AssertionError("search for %s did not end within %d draws" % (name, bound))


def _set_first(b, c, comp, inf=False, large=False, raw_bits=None):
    """byte string b with the flag bits of its first byte replaced"""
    b = bytearray(b)
    if raw_bits is None:
        if c is BN254:
            raw_bits = 0x40 if inf else (0xC0 if large else 0x80) if comp else 0
        else:
            raw_bits = (0x80 if comp else 0) | (0x40 if inf else 0) | (0x20 if large else 0)
    b[0] = (b[0] & flag_mask(c)) | raw_bits
    return bytes(b)


def _be(c, group, v):
    n = c.fp_bytes
    return v.to_bytes(n, "big") if group == 0 else v[1].to_bytes(n, "big") + v[0].to_bytes(n, "big")


@functools.lru_cache(maxsize=None)
def honest_points(cname, group):
    """[k]G for eight k: one, two, r - 1 and five seeded draws"""
    c = pyref.CURVES[cname]
    rng = pyref.Xoshiro(0xC0DEC + 2 * c.cid + group)
    G = group_of(c, group)
    return [G.mul(gen_of(c, group), k) for k in [1, 2, c.r - 1] + [rng.field(c.r) for _ in range(5)]]


@functools.lru_cache(maxsize=None)
def twist_real_points(cname):
    """G2 twist points whose x^3 + b' lies in Fp (the a1 = 0 arm of the Fp2 square root): x1 != 0 drawn, x0^2 = (x1^3 - b'_1) / (3 x1);
    one x whose real part t of x^3 + b' is a square, y = (s, 0), and one where it is not, y = (0, s) with s^2 = -t.  Curve points
    outside G2: the unchecked paths only need the curve."""
    c = pyref.CURVES[cname]
    p, rng = c.p, pyref.Xoshiro(0x7E157 + c.cid)
    F = pyref.Fp2Ops(p)

    def draw(_):
        x1 = rng.field(p - 1) + 1
        x0 = sqrt_fp((x1 ** 3 - c.b2[1]) * pow(3 * x1, -1, p) % p, p)
        if x0 is None:
            return None
        t = rhs_of(c, 1, (x0, x1))
        assert t[1] == 0
        return (x0, x1), t[0]

    out = []
    for want_square in (True, False):
        x, t = _search("a twist point with x^3 + b' in Fp", draw, lambda v: v is not None and v[1] != 0 and is_square_fp(v[1], p) == want_square)
        y = (sqrt_fp(t, p), 0) if want_square else (0, sqrt_fp(-t % p, p))
        assert F.mul(y, y) == (t, 0) and group_of(c, 1).on_curve((x, y))
        out.append((x, y))
    return out


@functools.lru_cache(maxsize=None)
def accept_cases(cname, group, compressed):
    c = pyref.CURVES[cname]
    G = group_of(c, group)
    out = []
    pts = [(("%dG" % i), P) for i, P in enumerate(honest_points(cname, group))]
    if group == 1:
        pts += [("twist-real-sq", twist_real_points(cname)[0]), ("twist-real-nonsq", twist_real_points(cname)[1])]
    for name, P in pts:
        for sign, Q in (("+", P), ("-", G.neg(P))):
            enc = encode_point(c, group, Q, compressed)
            out.append((name + sign, enc, Q))
            if compressed:   # the same bytes with the "largest" flag flipped: the other root, not a refusal
                large = is_largest(c, group, Q[1])
                out.append((name + sign + "-flipped", _set_first(enc, c, True, large=not large), G.neg(Q)))
    out.append(("infinity", encode_point(c, group, None, compressed), None))
    if not compressed:
        out.append(("all-zero", bytes(enc_len(c, group, False)), None))
    return out


@functools.lru_cache(maxsize=None)
def reject_cases(cname, group, compressed):
    """refused in a vector and as a header point alike -- but for the entries of other_mode_cases, which only a vector refuses"""
    c = pyref.CURVES[cname]
    p, n, cb, ln = c.p, c.fp_bytes, coord_bytes(c, group), enc_len(c, group, compressed)
    mask_bits = 254 if c is BN254 else 381
    rng = pyref.Xoshiro(0xBADC0DE + 4 * c.cid + 2 * group + compressed)
    G = group_of(c, group)
    fin = lambda b: _set_first(b, c, compressed)   # a finite point's flags (compressed: the smaller root; it never gets that far)
    out = []
    # a curve point whose leading x part leaves room for + p under the mask (about one x in three / four)
    lead = lambda P: P[0] if group == 0 else P[0][1]
    P = _search("a point with x + p under the mask", lambda i: G.mul(gen_of(c, group), rng.field(c.r)), lambda P: lead(P) + p < (1 << mask_bits))
    x, y = P
    good = encode_point(c, group, P, compressed)
    assert decode_point(c, group, good, compressed) == ("accept", P)

    def with_coords(xv, yv):   # integers (G2: pairs, A0 first) that may be >= p, under P's flags
        raw = b"".join(v.to_bytes(n, "big") for v in ((xv,) if group == 0 else (xv[1], xv[0])))
        if not compressed:
            raw += b"".join(v.to_bytes(n, "big") for v in ((yv,) if group == 0 else (yv[1], yv[0])))
        b = bytearray(raw)
        b[0] |= good[0] & ~flag_mask(c) & 0xFF
        return bytes(b)

    assert with_coords(x, y) == good
    if group == 0:
        out += [("x=p", with_coords(p, y)), ("x+p", with_coords(x + p, y))]
        if not compressed:
            out += [("y+p", with_coords(x, y + p)), ("y=p", with_coords(x, p))]
    else:
        out += [("A1=p", with_coords((x[0], p), y)), ("A0=p", with_coords((p, x[1]), y)), ("A1+p", with_coords((x[0], x[1] + p), y)),
                ("A0+p", with_coords((x[0] + p, x[1]), y))]
        if not compressed:
            out += [("yA1+p", with_coords(x, (y[0], y[1] + p))), ("yA0+p", with_coords(x, (y[0] + p, y[1])))]
    out.append(("all-ones", fin(b"\xff" * ln)))
    if group == 1:   # all ones in one half of x only
        out += [("A1-all-ones", fin(b"\xff" * n + good[n:])), ("A0-all-ones", good[:n] + b"\xff" * n + good[2 * n:])]
    # a canonical x that is no abscissa
    if group == 0:
        bad_x = _search("x with a non-residue x^3 + b", lambda i: rng.field(p), lambda v: not is_square_fp(rhs_of(c, 0, v), p))
    else:
        bad_x = _search("x with a non-residue x^3 + b'", lambda i: (rng.field(p), rng.field(p)), lambda v: sqrt_fp2(rhs_of(c, 1, v), p) is None)
    out.append(("non-residue", _set_first(_be(c, group, bad_x) + (b"" if compressed else _be(c, group, y)), c, compressed)))
    if not compressed:
        if group == 0:
            out += [("y+1", with_coords(x, (y + 1) % p)), ("y-1", with_coords(x, (y - 1) % p))]
        else:
            out += [("yA0+1", with_coords(x, ((y[0] + 1) % p, y[1]))), ("yA0-1", with_coords(x, ((y[0] - 1) % p, y[1]))),
                    ("yA1+1", with_coords(x, (y[0], (y[1] + 1) % p))), ("yA1-1", with_coords(x, (y[0], (y[1] - 1) % p)))]
    if c is BLS12_381:   # the malformed flag combinations, over a good x
        for bits in (0b001, 0b011, 0b111):
            out.append(("flags-%s" % bin(bits), _set_first(good, c, None, raw_bits=bits << 5)))
    # infinity with one stray bit
    inf = encode_point(c, group, None, compressed)
    places = [("byte0-low", 0, 0x01), ("x-middle", cb // 2, 0x10), ("last", ln - 1, 0x01)]
    if group == 1:
        places.append(("A0-first", n, 0x80))
    if not compressed:
        places += [("y-first", cb, 0x80), ("y-middle", cb + cb // 2, 0x04)]
    for name, at, bit in places:
        b = bytearray(inf)
        b[at] |= bit
        out.append(("infinity-stray-" + name, bytes(b)))
    return [(name, b, REJECT) for name, b in out]


@functools.lru_cache(maxsize=None)
def other_mode_cases(cname, group, compressed):
    """one stride of a `compressed` stream that carries the other mode's flags: refused inside a vector; a header point follows its own flag"""
    c = pyref.CURVES[cname]
    ln = enc_len(c, group, compressed)
    P = honest_points(cname, group)[3]
    other = encode_point(c, group, P, not compressed)
    out = [("other-mode-finite", (other + bytes(ln))[:ln])]
    if c is BLS12_381:
        out.append(("other-mode-infinity", bytes([0x40 if compressed else 0xC0]) + bytes(ln - 1)))
    return [(name, b, REJECT) for name, b in out]


def table(c, group, compressed):
    return accept_cases(c.name, group, compressed) + reject_cases(c.name, group, compressed) + other_mode_cases(c.name, group, compressed)


def test_reference_agrees_with_construction(c, group, compressed):
    """every seeded search ends within its bound (they run here), and the strict reference gives each case the verdict -- and the exact
    point -- it was built to have; BN254's infinity flag stays valid in both modes"""
    rows = table(c, group, compressed)
    for name, b, want in rows:
        got = decode_point(c, group, b, compressed)
        assert got == (REJECT if want == REJECT else ("accept", want)), name
    if c is BN254:
        assert decode_point(c, group, b"\x40" + bytes(enc_len(c, group, compressed) - 1), compressed) == ("accept", None)


# ---- 3. the two routes --------------------------------------------------------------------------------------------------------------------
def _arr(c, group, P):
    return pts_to_arr(c, group, [P])[0]


SENTINEL = 0xA5A5A5A5


def _point_unmarshal(lib, c, group, data):
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.full(len(_arr(c, group, None)), 0x1111111111111111, dtype=np.uint64)
    used = C.c_size_t(SENTINEL)
    rc = lib.ga_point_unmarshal(c.cid, group, buf.ctypes.data, buf.shape[0], out.ctypes.data, C.byref(used))
    return rc, out, used.value


def test_host_point_route(lib, c, group, compressed):
    """ga_point_unmarshal on every case, alone and with trailing bytes: a reject is GA_ERR_INVALID with `consumed` untouched, an accept
    gives the exact limbs and the exact `consumed` (the reference's: a header point follows its own flag)"""
    for name, b, _ in table(c, group, compressed):
        for data in (b, b + b"\x5a" * 7):
            want = decode_header(c, group, data, -1)
            rc, out, used = _point_unmarshal(lib, c, group, data)
            if want == REJECT:
                assert (rc, used) == (-1, SENTINEL), (name, len(data))
            else:
                assert rc == 0 and used == want[2] and np.array_equal(out, _arr(c, group, want[1])), (name, len(data))


def _proof_unmarshal(lib, c, data):
    fp = c.fp_limbs
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    out, coms, pok = np.zeros(8 * fp, dtype=np.uint64), np.zeros((4, 2 * fp), dtype=np.uint64), np.zeros(2 * fp, dtype=np.uint64)
    n, used = C.c_uint32(SENTINEL), C.c_size_t(SENTINEL)
    rc = lib.ga_g16_proof_unmarshal(c.cid, buf.ctypes.data, buf.shape[0], out.ctypes.data, coms.ctypes.data, 4, C.byref(n), pok.ctypes.data, C.byref(used))
    return rc, out, coms, pok, n.value, used.value


def test_host_proof_route(lib, c, group, compressed):
    """ga_g16_proof_unmarshal with the case as Ar, Krs, the commitment and the PoK (G1) or as Bs (G2) of a proof whose other points are
    honest and of the same mode: verdict, every limb and `consumed` are the strict proof reader's"""
    h1, h2 = honest_points(c.name, 0), honest_points(c.name, 1)
    fp = c.fp_limbs
    for name, b, _ in table(c, group, compressed):
        for slot in ((0, 2, 3, 4) if group == 0 else (1,)):
            parts = [encode_point(c, 0, h1[4], compressed), encode_point(c, 1, h2[4], compressed), encode_point(c, 0, h1[5], compressed),
                     encode_point(c, 0, h1[6], compressed), encode_point(c, 0, h1[7], compressed)]
            parts[slot] = b
            data = parts[0] + parts[1] + parts[2] + (1).to_bytes(4, "big") + parts[3] + parts[4] + b"tail"
            want = decode_proof(c, data, 4)
            rc, out, coms, pok, n, used = _proof_unmarshal(lib, c, data)
            if want == REJECT:
                assert (rc, used, n) == (-1, SENTINEL, SENTINEL), (name, slot)
                continue
            _, ar, bs, krs, cm, pk_, consumed = want
            assert rc == 0 and used == consumed and n == len(cm), (name, slot)
            assert np.array_equal(out, np.concatenate([_arr(c, 0, ar), _arr(c, 1, bs), _arr(c, 0, krs)])), (name, slot)
            assert np.array_equal(coms[:n], pts_to_arr(c, 0, cm).reshape(n, 2 * fp)) and np.array_equal(pok, _arr(c, 0, pk_)), (name, slot)


# the device route: the logn = 7 synthetic key (126 or 127 points per vector), cases in place of entries of G1.A, G1.K and G2.B
_INST = {}


def instance(ctx, c, logn=7):
    """(synthetic instance, the same key as a pyref.ProvingKey), made once per context"""
    key = (id(ctx), c.cid, logn)
    if key not in _INST:
        inst = synth.make_instance(ctx, c.name, logn, 0xC0DEC0 + c.cid, want_dlogs=False)
        k = inst.key
        g1 = lambda a: [arr_to_g1_affine(c, row) for row in a]
        g2 = lambda a: [arr_to_g2_affine(c, row) for row in a]
        pk = pyref.ProvingKey(curve=c, n=inst.n, alpha1=g1(k["alpha1"])[0], beta1=g1(k["beta1"])[0], delta1=g1(k["delta1"])[0], A=g1(k["A"]),
                              B=g1(k["B"]), Z=g1(k["Z"]), K=g1(k["K"]), beta2=g2(k["beta2"])[0], delta2=g2(k["delta2"])[0], B2=g2(k["B2"]),
                              infinityA=[int(v) for v in k["infinityA"]], infinityB=[int(v) for v in k["infinityB"]])
        _INST[key] = (inst, pk)
    return _INST[key]


def key_fields(c, pk):
    return dict(domain_cardinality=pk.n, alpha1=pts_to_arr(c, 0, [pk.alpha1]), beta1=pts_to_arr(c, 0, [pk.beta1]),
                delta1=pts_to_arr(c, 0, [pk.delta1]), A=pts_to_arr(c, 0, pk.A), B=pts_to_arr(c, 0, pk.B), Z=pts_to_arr(c, 0, pk.Z),
                K=pts_to_arr(c, 0, pk.K), beta2=pts_to_arr(c, 1, [pk.beta2]), delta2=pts_to_arr(c, 1, [pk.delta2]),
                B2=pts_to_arr(c, 1, pk.B2), infinityA=np.array(pk.infinityA, dtype=np.uint8), infinityB=np.array(pk.infinityB, dtype=np.uint8))


def vector_offset(c, pk, raw, which, index=0):
    """byte offset of point `index` of vector `which` (A B Z K B2) in pk_write(pk, raw) (with the withPrecompute byte, no commitments)"""
    s1, s2 = enc_len(c, 0, not raw), enc_len(c, 1, not raw)
    off = 8 + 160 + 1 + 3 * s1
    for name in ("A", "B", "Z", "K"):
        if name == which:
            return off + 4 + index * s1
        off += 4 + s1 * len(getattr(pk, name))
    assert which == "B2"
    return off + 2 * s2 + 4 + index * s2


def planted_image(c, pk, raw, plant):
    """pk_write(pk, raw) with the bytes of plant[(vector, index)] in place of those points"""
    img = bytearray(pyref.pk_write(pk, raw=raw))
    for (which, index), b in plant.items():
        off = vector_offset(c, pk, raw, which, index)
        assert len(b) == enc_len(c, int(which == "B2"), not raw)
        img[off:off + len(b)] = b
    return bytes(img)


def read_key(ctx, c, source, **kw):
    """ProvingKey.ReadFrom with the vectors left as they are read (precompute = -1: no tables, which the codec has no part in)"""
    return groth16.ProvingKey.ReadFrom(ctx, c.name, source, precompute=-1, **kw)


def _prove(dpk, inst):
    try:
        return groth16.Prove(dpk, inst.solution, inst.nb_public, inst.r, inst.s).raw()
    finally:
        dpk.FreeGPUResources()


def test_device_route(ctx, c, compressed):
    """the cases inside a key read by ProvingKey.ReadFrom from memory: all accept cases at once in G1.A, G1.K (from index 3 and from the
    end backwards) and G2.B -- the key proves to the bytes of the key built from host arrays of the REFERENCE's points; then, vector by
    vector, every reject case at once: "k of n points do not decode" with exactly that k"""
    inst, pk = instance(ctx, c)
    raw = not compressed
    acc1, acc2 = accept_cases(c.name, 0, compressed), accept_cases(c.name, 1, compressed)
    assert len(acc1) + 3 <= len(pk.A) and len(acc2) + 3 <= len(pk.B2)
    plant, vec = {}, {"A": list(pk.A), "K": list(pk.K), "B2": list(pk.B2)}
    for which, rows, group, at in (("A", acc1, 0, lambda i: 3 + i), ("K", acc1, 0, lambda i: len(pk.K) - 1 - i), ("B2", acc2, 1, lambda i: 3 + i)):
        for i, (_, b, _) in enumerate(rows):
            v = decode_point(c, group, b, compressed)
            plant[(which, at(i))] = b
            vec[which][at(i)] = v[1]
    want_pk = dataclasses.replace(pk, A=vec["A"], K=vec["K"], B2=vec["B2"])
    want = _prove(groth16.ProvingKey(ctx, c.name, precompute=-1, **key_fields(c, want_pk)), inst)
    assert not np.array_equal(want, _prove(inst.proving_key(ctx, precompute=-1), inst))
    img = planted_image(c, pk, raw, plant)
    dpk = read_key(ctx, c, img)
    assert dpk.bytes_read == len(img)
    assert np.array_equal(_prove(dpk, inst), want)
    for which, group in (("A", 0), ("K", 0), ("B2", 1)):
        rej = reject_cases(c.name, group, compressed) + other_mode_cases(c.name, group, compressed)
        n = len(getattr(pk, which))
        assert all(decode_point(c, group, b, compressed) == REJECT for _, b, _ in rej) and 2 * len(rej) < n
        bad = planted_image(c, pk, raw, {(which, 2 * i + 1): b for i, (_, b, _) in enumerate(rej)})
        with pytest.raises(GnarkAmdError, match=r"error -1: .*key file: %d of %d points do not decode" % (len(rej), n)):
            read_key(ctx, c, bad)
    read_key(ctx, c, pyref.pk_write(pk, raw=raw)).FreeGPUResources()   # and the reader is usable afterwards


# ---- encode thresholds: point_encode does not test the curve equation, so any affine pair will do ------------------------------------------
def threshold_images(c, group):
    p = c.p
    four = [1, (p - 1) // 2, (p + 1) // 2, p - 1]
    if group == 0:
        return [(7, y) for y in four]
    return [((7, 9), (y0, 0)) for y0 in four] + [((7, 9), (y0, y1)) for y0 in (1, p - 1) for y1 in four]


def _largest_bit(c, b0):
    return (b0 >> 6) == 3 if c is BN254 else bool(b0 & 0x20)


def test_encode_thresholds_host(lib, c):
    """ga_g16_proof_marshal / _bsb22 / _raw: y = (p - 1) / 2 is the smaller root, (p + 1) / 2 the larger; in Fp2 A1 decides and A0 only
    when A1 = 0; the bytes are the reference encoder's"""
    half = (c.p - 1) // 2
    im1, im2 = threshold_images(c, 0), threshold_images(c, 1)
    for i, Q in enumerate(im2):
        ar, krs, cm, pok = im1[i % 4], im1[(i + 1) % 4], im1[(i + 2) % 4], im1[(i + 3) % 4]
        proof = groth16.Proof(c.cid, _arr(c, 0, ar), _arr(c, 1, Q), _arr(c, 0, krs), lib)
        got = proof.WriteTo()
        want_large = (Q[1][1] > half) if Q[1][1] else (Q[1][0] > half)
        assert _largest_bit(c, got[c.fp_bytes]) == want_large and _largest_bit(c, got[0]) == (ar[1] > half), i
        assert got == b"".join([encode_point(c, 0, ar, True), encode_point(c, 1, Q, True), encode_point(c, 0, krs, True), bytes(4),
                                encode_point(c, 0, None, True)]), i
        proof.Commitments, proof.CommitmentPok = pts_to_arr(c, 0, [cm]), _arr(c, 0, pok)
        for raw, got in ((False, proof.WriteTo()), (True, proof.WriteRawTo())):
            assert got == b"".join([encode_point(c, 0, ar, not raw), encode_point(c, 1, Q, not raw), encode_point(c, 0, krs, not raw),
                                    (1).to_bytes(4, "big"), encode_point(c, 0, cm, not raw), encode_point(c, 0, pok, not raw)]), (i, raw)


def test_encode_thresholds_device(ctx, c):
    """the same images through key_encode_kernel: WriteKey, compressed, with them as G1.A and G2.B"""
    inst, pk = instance(ctx, c)
    im1, im2 = threshold_images(c, 0), threshold_images(c, 1)
    tpk = dataclasses.replace(pk, A=im1 + list(pk.A[len(im1):]), B2=im2 + list(pk.B2[len(im2):]))
    with tempfile.TemporaryFile() as f:
        groth16.WriteKey(ctx, c.name, f, groth16.KEY_FORMAT_COMPRESSED, **key_fields(c, tpk))
        f.seek(0)
        img = f.read()
    half = (c.p - 1) // 2
    for which, group, ims in (("A", 0, im1), ("B2", 1, im2)):
        for i, Q in enumerate(ims):
            off = vector_offset(c, tpk, False, which, i)
            y = Q[1]
            want_large = y > half if group == 0 else (y[1] > half if y[1] else y[0] > half)
            assert _largest_bit(c, img[off]) == want_large, (which, i)
            assert img[off:off + enc_len(c, group, True)] == encode_point(c, group, Q, True), (which, i)


# ---- 4. multi-pass streams: GA_KEY_CHUNK ------------------------------------------------------------------------------------------------------
class chunk_knob:
    def __init__(self, monkeypatch, value):
        self.mp, self.value = monkeypatch, value

    def __enter__(self):
        if self.value is None:
            self.mp.delenv("GA_KEY_CHUNK", raising=False)
        else:
            self.mp.setenv("GA_KEY_CHUNK", str(self.value))

    def __exit__(self, *exc):
        self.mp.delenv("GA_KEY_CHUNK", raising=False)


@functools.lru_cache(maxsize=None)
def _images_cached(cname, key_id):
    pk = _PKS[key_id]
    return {"compressed": pyref.pk_write(pk, raw=False), "raw": pyref.pk_write(pk, raw=True), "dump": pyref.pk_write_dump(pk)}


_PKS = {}


def images(c, pk):
    _PKS[id(pk)] = pk
    return _images_cached(c.name, id(pk))


def reference_proof(ctx, c):
    inst, _ = instance(ctx, c)
    key = ("proof", id(ctx), c.cid)
    if key not in _INST:
        _INST[key] = _prove(inst.proving_key(ctx, precompute=-1), inst)
    return _INST[key]


def test_multipass_read_write(ctx, monkeypatch, c, knob, tmp_path):
    """the three formats written (bytes == pyref.pk_write / pk_write_dump) and read from memory and from a descriptor (proof == the
    host-array key's), with `knob` points per staging pass"""
    inst, pk = instance(ctx, c)
    want = reference_proof(ctx, c)
    with chunk_knob(monkeypatch, knob):
        for fmt, img in images(c, pk).items():
            path = tmp_path / ("key_%s.bin" % fmt)
            with open(path, "wb") as f:
                n = groth16.WriteKey(ctx, c.name, f, FORMATS[fmt], **inst.key, domain_cardinality=inst.n)
            assert n == len(img) and open(path, "rb").read() == img, fmt
            dpk = read_key(ctx, c, img)
            assert dpk.bytes_read == len(img)
            assert np.array_equal(_prove(dpk, inst), want), (fmt, "mem")
            with open(path, "rb") as f:
                dpk = read_key(ctx, c, f)
            assert dpk.bytes_read == len(img)
            assert np.array_equal(_prove(dpk, inst), want), (fmt, "fd")


def test_multipass_shards(ctx, monkeypatch, c, knob):
    """shards (0, 2) and (1, 2), and the three of 3 twice -- (1, 3) keeps [42, 84) of 126, a window that begins and ends inside a pass of
    63 .. 65 points -- each shard from another format, so that every format serves (1, 3) or (1, 2): the summed partials finish to the
    reference proof"""
    inst, pk = instance(ctx, c)
    want = reference_proof(ctx, c)
    img = images(c, pk)
    with chunk_knob(monkeypatch, knob):
        for fmts in (("compressed", "dump"), ("raw", "compressed", "dump"), ("dump", "raw", "compressed")):
            parts, count = [], len(fmts)
            for k, fmt in enumerate(fmts):
                spk = read_key(ctx, c, img[fmt], shard=(k, count))
                try:
                    parts.append(groth16.ProvePartial(spk, inst.solution, inst.nb_public))
                    if k == count - 1:
                        fin = groth16.Finish(spk, groth16.SumPartials(c.name, parts, lib=ctx.lib), inst.r, inst.s).raw()
                finally:
                    spk.FreeGPUResources()
            assert np.array_equal(fin, want), fmts


def _read_from_pipe(ctx, c, data):
    """ProvingKey.ReadFrom on the read end of a pipe that a thread fills with `data` and closes"""
    import threading
    r, w = os.pipe()

    def feed():
        try:
            with os.fdopen(w, "wb") as f:
                f.write(data)
        except BrokenPipeError:
            pass

    t = threading.Thread(target=feed)
    t.start()
    try:
        with os.fdopen(r, "rb", buffering=0) as f:
            return read_key(ctx, c, f)
    finally:
        t.join()


# not in the first pass for 1, 63, 64 or 65 points per pass; shard 1 of 2 keeps it, and so does shard 2 of 3, whose window [84, 126) begins
# inside the pass that holds it; shard 0 of 2 does not
BAD_INDEX = 100


def test_multipass_checked_reads(ctx, monkeypatch, c, knob):
    """one point replaced by P + [r]Q (G2.B; on BLS12-381 G1.A as well) at index 100, in a later pass: the checked read names the vector
    and that file index, in every format, whole (the dump) or as a shard that keeps it -- (1, 2) and (2, 3), whose window [84, 126) begins
    inside the pass that holds the point; the shard that does not keep it accepts; a checked read
    of the good bytes succeeds afterwards"""
    from test_check_points import random_curve_point
    inst, pk = instance(ctx, c)
    rng = pyref.Xoshiro(0x0C4EC + c.cid)
    G1, G2 = group_of(c, 0), group_of(c, 1)
    swap = lambda v, P: v[:BAD_INDEX] + [P] + v[BAD_INDEX + 1:]
    key = ("bad", c.cid)
    if key not in _INST:   # (independent of the context: points and bytes only)
        out2 = G2.add(pk.B2[BAD_INDEX], G2.mul(random_curve_point(c, 1, rng), c.r))
        rows = [(dataclasses.replace(pk, B2=swap(pk.B2, out2)), r"G2\.B")]
        if c is BLS12_381:
            out1 = G1.add(pk.A[BAD_INDEX], G1.mul(random_curve_point(c, 0, rng), c.r))
            rows.append((dataclasses.replace(pk, A=swap(pk.A, out1)), r"G1\.A"))
        _INST[key] = rows
    # (a checked pass of one point costs a whole launch chain of the subgroup test: the reads below keep a third or a half of the file)
    refused = {"compressed": ((2, 3),), "raw": ((1, 2),), "dump": ((0, 1),)}
    accepted = {"compressed": (0, 3), "dump": (0, 2)}
    with chunk_knob(monkeypatch, knob):
        for bad_pk, vector in _INST[key]:
            where = r"error -1: .*point %d of %s is not in the prime-order subgroup" % (BAD_INDEX, vector)
            for fmt, img in images(c, bad_pk).items():
                for shard in refused[fmt]:
                    with pytest.raises(GnarkAmdError, match=where):
                        read_key(ctx, c, img, shard=shard, subgroup_check=True)
                if fmt in accepted:
                    read_key(ctx, c, img, shard=accepted[fmt], subgroup_check=True).FreeGPUResources()
        read_key(ctx, c, images(c, pk)["compressed"], shard=(1, 3), subgroup_check=True).FreeGPUResources()
        read_key(ctx, c, images(c, pk)["dump"], subgroup_check=True).FreeGPUResources()


def test_multipass_undecodable_and_truncation(ctx, monkeypatch, c, knob):
    """the logn = 8 key (254 points in G1.A): three undecodable points in three different passes for every knob value but unset -- A[10],
    A[70], A[140]; the last pass is clean -- are "3 of 254", compressed and raw; input cut inside the second pass of G1.A is "end of
    input", from memory (where the length word is checked against what is left) and from a pipe (where the second pass runs dry)"""
    inst, pk = instance(ctx, c, 8)
    na = len(pk.A)
    assert na == 254
    with chunk_knob(monkeypatch, knob):
        for compressed in (True, False):
            stray = bytearray(encode_point(c, 0, None, compressed))
            stray[-1] |= 2
            rej = reject_cases(c.name, 0, compressed)
            plant = {("A", 10): bytes(stray), ("A", 70): rej[0][1], ("A", 140): [b for name, b, _ in rej if name == "non-residue"][0]}
            with pytest.raises(GnarkAmdError, match=r"error -1: .*key file: 3 of %d points do not decode" % na):
                read_key(ctx, c, planted_image(c, pk, not compressed, plant))
        per = knob or 64
        for fmt, img in images(c, pk).items():
            if fmt == "dump":   # the slices come last: G1.A's begins where the other four and theirs length words end
                rest = sum(8 + 16 * c.fp_limbs * len(v) for v in (pk.B, pk.Z, pk.K)) + 8 + 32 * c.fp_limbs * len(pk.B2)
                cut = len(img) - rest - (na - per - per // 2) * 16 * c.fp_limbs + 5
            else:
                cut = vector_offset(c, pk, fmt == "raw", "A", per + per // 2) + 5
            if fmt == "compressed":
                with pytest.raises(GnarkAmdError, match="end of input"):
                    read_key(ctx, c, img[:cut])
            with pytest.raises(GnarkAmdError, match="end of input"):
                _read_from_pipe(ctx, c, img[:cut])
        good = images(c, pk)["compressed"]
        dpk = read_key(ctx, c, good)
        assert dpk.bytes_read == len(good)
        dpk.FreeGPUResources()

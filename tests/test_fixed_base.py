"""Fixed-base batch scalar multiplication (ga_batch_scalar_mul: curve.BatchScalarMultiplicationG1 / G2 of groth16.Setup,
backend/groth16/bn254/setup.go:233,302, and kzg.NewSRS) on the functional emulation.  Every case is a function of a context;
tests/test_fixed_base_gpu.py runs the same cases on the device."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle
import pyref
from gnark_amd import _lib, ecc, groth16
from gnark_amd._lib import GnarkAmdError
from gnark_amd.device import affine_words
from helpers import BLS12_381, BN254, fr_to_arr, gen_of, group_of, pts_to_arr

CURVES = [BN254, BLS12_381]
SIZES = (1, 2, 63, 64, 65, 257, 1000)
WIDTHS = (4, 7, 13)

# expected points, computed once per (curve, group, scalar) and shared by every width, size and placement
_EXPECT = {}


def _one_expected(cid, group, k):
    return oracle.jac_to_affine(cid, group, oracle.generator_mul(cid, group, k))


def expected_points(c, group, ks):
    """oracle.generator_mul + oracle.jac_to_affine per scalar, as an (n, affine_words) array"""
    todo = sorted({k for k in ks if (c.cid, group, k) not in _EXPECT})
    if len(todo) > 4096:   # (the C oracle releases the interpreter lock: a few threads for the 2^16 case)
        with ThreadPoolExecutor(16) as ex:
            rows = list(ex.map(lambda k: _one_expected(c.cid, group, k), todo, chunksize=256))
    else:
        rows = [_one_expected(c.cid, group, k) for k in todo]
    for k, row in zip(todo, rows):
        _EXPECT[(c.cid, group, k)] = row
    return np.stack([_EXPECT[(c.cid, group, k)] for k in ks])


def window_count(c, width):
    return c.r.bit_length() // width + 1


def edge_scalars(c, width):
    r = c.r
    e = [0, 1, 2, r - 1, r - 2, 1 << (width - 1), (1 << width) - 1, 1 << width]
    for j in range(window_count(c, width)):
        e += [((1 << (width * j)) + 1) % r, ((1 << (width * j)) - 1) % r]
    e.append((1 << 253) - 1)
    return e


def scalars_for(c, n, width):
    """n random scalars (the same for every width) with the edge scalars of `width` at positions 0, 1, ... as far as they fit"""
    rng = pyref.Xoshiro(0xF1BA5E + 7919 * n + c.cid)
    ks = [rng.field(c.r) for _ in range(n)]
    edges = edge_scalars(c, width)
    ks[:min(n, len(edges))] = edges[:n]
    return ks


def canon(c, ks):
    return fr_to_arr(c, ks, mont=False)


def gen_arr(c, group):
    return pts_to_arr(c, group, [gen_of(c, group)])


class knobs:
    """GA_FIXED_BASE_C / GA_FIXED_BASE_CHUNK / GA_MSM_EXACT_REDO for the calls inside the block (read once per entry point)"""

    def __init__(self, monkeypatch, width=None, chunk=None, exact=False):
        self.mp, self.env = monkeypatch, {"GA_FIXED_BASE_C": width, "GA_FIXED_BASE_CHUNK": chunk, "GA_MSM_EXACT_REDO": 1 if exact else None}

    def __enter__(self):
        for k, v in self.env.items():
            if v is None:
                self.mp.delenv(k, raising=False)
            else:
                self.mp.setenv(k, str(v))

    def __exit__(self, *a):
        for k in self.env:
            self.mp.delenv(k, raising=False)


# ---- 1. point for point against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_fixed_base_vs_oracle(emu_ctx, monkeypatch, c, group, width, sizes=SIZES):
    """generator base, n in {1, 2, 63, 64, 65, 257, 1000}, random + edge scalars, forced window width: every point equals
    oracle.generator_mul; canonical == Montgomery scalars, host == device placement of scalars and output, byte for byte"""
    ctx, base = emu_ctx, gen_arr(c, group)
    wa = affine_words(c.cid, group)
    with knobs(monkeypatch, width=width):
        for n in sizes:
            # (the edge scalars sit on the window boundaries of the width the library really uses: the forced one, else the planned one)
            ks = scalars_for(c, n, width if width else ecc.batch_scalar_mul_plan(c.name, n, lib=ctx.lib)[0])
            want = expected_points(c, group, ks)
            got = ecc.BatchScalarMultiplication(ctx, c.name, group, base, canon(c, ks))
            assert got.shape == (n, wa)
            bad = np.where((got != want).any(axis=1))[0]
            assert bad.size == 0, (n, width, bad[:8], [hex(ks[i]) for i in bad[:4]])
            if n in (2, 257, 1000, max(sizes)):
                mont = ecc.BatchScalarMultiplication(ctx, c.name, group, base, fr_to_arr(c, ks), montgomery=True)
                assert np.array_equal(mont, want), (n, "montgomery")
            if n in (65, 1000, max(sizes)):   # placements: device scalars -> host output, device scalars -> device output, host -> device
                d_s = ctx.to_device(canon(c, ks))
                try:
                    assert np.array_equal(ecc.BatchScalarMultiplication(ctx, c.name, group, base, d_s, n=n), want)
                    for src in (d_s, canon(c, ks)):
                        d_o = ecc.BatchScalarMultiplication(ctx, c.name, group, base, src, n=n, out_device=True)
                        try:
                            assert np.array_equal(d_o.to_host((n, wa)), want)
                        finally:
                            d_o.free()
                finally:
                    d_s.free()


# ---- 2. other bases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_fixed_base_other_bases(emu_ctx, monkeypatch, c, group):
    """a random multiple of the generator as base vs pyref's Group.mul (n = 32); base (0,0): every output (0,0); a base off the
    curve: GA_ERR_INVALID, and the context keeps working; n = 0 and the other argument errors"""
    ctx, Gp, n = emu_ctx, group_of(c, group), 32
    wa = affine_words(c.cid, group)
    rng = pyref.Xoshiro(0xBA5E + group)
    B = Gp.mul(gen_of(c, group), rng.field(c.r))
    ks = [rng.field(c.r) for _ in range(n)]
    ks[:4] = [0, 1, c.r - 1, 2]
    want = pts_to_arr(c, group, [Gp.mul(B, k) for k in ks])
    for width in (5, None):
        with knobs(monkeypatch, width=width):
            assert np.array_equal(ecc.BatchScalarMultiplication(ctx, c.name, group, pts_to_arr(c, group, [B]), canon(c, ks)), want), width
    inf = np.zeros((1, wa), np.uint64)
    assert not ecc.BatchScalarMultiplication(ctx, c.name, group, inf, canon(c, ks)).any()
    off = pts_to_arr(c, group, [B]).copy()
    off[0, 0] ^= np.uint64(2)   # (x changed, y kept: not on the curve)
    with pytest.raises(GnarkAmdError):
        ecc.BatchScalarMultiplication(ctx, c.name, group, off, canon(c, ks))
    assert np.array_equal(ecc.BatchScalarMultiplication(ctx, c.name, group, pts_to_arr(c, group, [B]), canon(c, ks)), want)
    # n = 0 is GA_OK and touches nothing; unknown curve / group, null pointers with n > 0
    lib, h = ctx.lib, ctx.handle
    assert lib.ga_batch_scalar_mul(h, c.cid, group, None, None, 0, 0, None) == 0
    assert ecc.BatchScalarMultiplication(ctx, c.name, group, inf, np.zeros((0, 4), np.uint64)).shape == (0, wa)
    out, s1 = np.zeros((1, wa), np.uint64), canon(c, [1])
    P = lambda a: a.ctypes.data
    assert lib.ga_batch_scalar_mul(h, 7, group, P(inf), P(s1), 1, 0, P(out)) == -1
    assert lib.ga_batch_scalar_mul(h, c.cid, 2, P(inf), P(s1), 1, 0, P(out)) == -1
    assert lib.ga_batch_scalar_mul(h, c.cid, group, None, P(s1), 1, 0, P(out)) == -1
    assert lib.ga_batch_scalar_mul(h, c.cid, group, P(inf), None, 1, 0, P(out)) == -1
    assert lib.ga_batch_scalar_mul(h, c.cid, group, P(inf), P(s1), 1, 0, None) == -1


# ---- 3. every addition exceptional ---------------------------------------------------------------------------------------------
def order3_point():
    """a point of order 3 on BLS12-381 G1 (the cofactor (z - 1)^2 / 3 is divisible by 3): T = [h r / 3](x, y)"""
    c = BLS12_381
    Gp = pyref.g1_group(c)
    z = -0xd201000000010000
    h = (z - 1) ** 2 // 3
    assert h % 3 == 0
    rng = pyref.Xoshiro(0x0DD3)
    while True:
        x = rng.field(c.p)
        y = pyref._sqrt_fp((x * x * x + 4) % c.p, c.p)
        if y is None or y * y % c.p != (x * x * x + 4) % c.p:
            continue
        T = Gp.mul((x, y), h * c.r // 3)
        if T is not None:
            break
    assert Gp.on_curve(T) and Gp.mul(T, 3) is None
    return T


@pytest.mark.parametrize("exact", [False, True], ids=["complete-lazy", "exact-kernel"])
def test_fixed_base_order3_base(emu_ctx, monkeypatch, exact):
    """base of order 3, 200 random scalars: table entries at infinity, doublings and P + (-P) in every lane -- the redo path (the
    complete lazy loop; with GA_MSM_EXACT_REDO=1 the exact kernel) carries the whole result: outputs == [s mod 3] T"""
    c, n = BLS12_381, 200
    Gp, T = pyref.g1_group(c), order3_point()
    rng = pyref.Xoshiro(0x3333)
    ks = [rng.field(c.r) for _ in range(n)]
    want = pts_to_arr(c, 0, [Gp.mul(T, k % 3) for k in ks])
    assert len({tuple(row) for row in want}) == 3   # infinity, T and -T all occur
    for width in (4, 7):
        with knobs(monkeypatch, width=width, exact=exact):
            got = ecc.BatchScalarMultiplication(emu_ctx, c.name, 0, pts_to_arr(c, 0, [T]), canon(c, ks))
        assert np.array_equal(got, want), width


# ---- 4. chunking and bit reversal ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,group", [(BN254, 0), (BLS12_381, 1)], ids=["bn254-G1", "bls12-381-G2"])
def test_fixed_base_chunks_and_bitreversal(emu_ctx, monkeypatch, c, group):
    """n = 1000 and 4096 in chunks of 256 == one chunk; GA_RESULT_BITREVERSED at n = 1, 2, 1024 == numpy's permutation (host and
    device output, one chunk and four); n = 1000 with the flag: GA_ERR_INVALID"""
    ctx, base = emu_ctx, gen_arr(c, group)
    wa = affine_words(c.cid, group)
    rng = pyref.Xoshiro(0xC4C4 + group)
    ks = [rng.field(c.r) for _ in range(4096)]
    S = canon(c, ks)
    with knobs(monkeypatch, width=7):
        whole = ecc.BatchScalarMultiplication(ctx, c.name, group, base, S)
    assert np.array_equal(whole[:64], expected_points(c, group, ks[:64]))
    for n in (1000, 4096):
        with knobs(monkeypatch, width=7, chunk=256):
            assert np.array_equal(ecc.BatchScalarMultiplication(ctx, c.name, group, base, S[:n]), whole[:n]), n
            d_o = ecc.BatchScalarMultiplication(ctx, c.name, group, base, S[:n], out_device=True)
            try:
                assert np.array_equal(d_o.to_host((n, wa)), whole[:n]), n
            finally:
                d_o.free()
    for n in (1, 2, 1024):
        logn = n.bit_length() - 1
        perm = np.array([pyref.bitrev(i, logn) for i in range(n)])
        want = np.empty((n, wa), np.uint64)
        want[perm] = whole[:n]
        for chunk in (None, 256):
            with knobs(monkeypatch, width=7, chunk=chunk):
                assert np.array_equal(ecc.BatchScalarMultiplication(ctx, c.name, group, base, S[:n], bitreversed=True), want), (n, chunk)
                d_o = ecc.BatchScalarMultiplication(ctx, c.name, group, base, S[:n], bitreversed=True, out_device=True)
                try:
                    assert np.array_equal(d_o.to_host((n, wa)), want), (n, chunk)
                finally:
                    d_o.free()
    with pytest.raises(GnarkAmdError):
        ecc.BatchScalarMultiplication(ctx, c.name, group, base, S[:1000], bitreversed=True)


# ---- 5. the reference's use, end to end ----------------------------------------------------------------------------------------
def device_key(ctx, c, cs, toxic):
    """groth16.Setup's two BatchScalarMultiplication calls (setup.go:233,302) on the device: the key's point vectors from the scalars"""
    pk, vk, dlog = pyref.groth16_setup(c, cs, toxic)
    delta, tau = toxic[3], toxic[4]
    g1, g2 = gen_arr(c, 0), gen_arr(c, 1)
    bsm = lambda group, ks, **kw: ecc.BatchScalarMultiplication(ctx, c.name, group, g2 if group else g1, canon(c, ks), **kw)
    tn1 = (pow(tau, pk.n, c.r) - 1) % c.r
    zs = [pow(tau, i, c.r) * tn1 % c.r * pow(delta, -1, c.r) % c.r for i in range(pk.n)]   # natural order (setup.go:181-192)
    dev = dict(A=bsm(0, dlog["A"]), B=bsm(0, dlog["B"]), K=bsm(0, dlog["K"]), B2=bsm(1, dlog["B"]),
               Z=bsm(0, zs, bitreversed=True)[:pk.n - 1])
    return pk, vk, dev


@pytest.mark.parametrize("circuit", ["cubic", "commit"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_fixed_base_reproduces_groth16_key(emu_ctx, c, circuit):
    """pyref.groth16_setup with fixed toxic waste: pk.A, pk.B, pk.K, pk.B2 from dlog's scalars, pk.Z from the natural-order Z
    scalars with the bit-reversed flag (n - 1 points kept) -- point for point; cubic: a proof made with the key assembled from
    the device outputs is accepted by pyref.groth16_verify"""
    ctx = emu_ctx
    rng = pyref.Xoshiro(0x5E7 + c.cid)
    cs = pyref.cubic_r1cs() if circuit == "cubic" else pyref.commit_r1cs()
    toxic = [rng.field(c.r) for _ in range(5 + len(cs.commitments) + 1)]
    pk, vk, dev = device_key(ctx, c, cs, toxic)
    for name, group in (("A", 0), ("B", 0), ("K", 0), ("Z", 0), ("B2", 1)):
        assert np.array_equal(dev[name], pts_to_arr(c, group, getattr(pk, name))), name
    if circuit != "cubic":
        return
    w = pyref.cubic_witness(3)
    A, B, Cc = pyref.r1cs_solve(c, cs, w)
    r, s = rng.field(c.r), rng.field(c.r)
    dpk = groth16.ProvingKey(
        ctx, c.name, domain_cardinality=pk.n, alpha1=pts_to_arr(c, 0, [pk.alpha1]), beta1=pts_to_arr(c, 0, [pk.beta1]),
        delta1=pts_to_arr(c, 0, [pk.delta1]), A=dev["A"], B=dev["B"], Z=dev["Z"], K=dev["K"], beta2=pts_to_arr(c, 1, [pk.beta2]),
        delta2=pts_to_arr(c, 1, [pk.delta2]), B2=dev["B2"], infinityA=pk.infinityA, infinityB=pk.infinityB)
    try:
        proof = groth16.Prove(dpk, groth16.Solution(W=fr_to_arr(c, w), A=fr_to_arr(c, A), B=fr_to_arr(c, B), C=fr_to_arr(c, Cc)),
                              cs.nb_public, fr_to_arr(c, [r]), fr_to_arr(c, [s]))
    finally:
        dpk.FreeGPUResources()
    got = pyref.proof_read(c, proof.WriteTo())[:5]
    assert pyref.groth16_verify(c, vk, got, w[1:cs.nb_public])
    assert not pyref.groth16_verify(c, vk, got, [(w[1] ^ 1) % c.r])


def test_fixed_base_plan(emu_lib, monkeypatch):
    """ga_batch_scalar_mul_plan: deterministic, windows = BITS / c + 1, wider for more scalars, the forced width when the knob is set"""
    with knobs(monkeypatch):
        for c in CURVES:
            plans = [ecc.batch_scalar_mul_plan(c.name, 1 << ln, lib=emu_lib) for ln in (0, 10, 16, 20, 24, 30)]
            assert plans == [ecc.batch_scalar_mul_plan(c.name, 1 << ln, lib=emu_lib) for ln in (0, 10, 16, 20, 24, 30)]
            assert all(4 <= w <= 18 and nw == window_count(c, w) for w, nw in plans), plans
            assert [w for w, _ in plans] == sorted(w for w, _ in plans) and plans[0][0] < plans[-1][0], plans
    for forced in (2, 13, 20):
        with knobs(monkeypatch, width=forced):
            assert ecc.batch_scalar_mul_plan("bn254", 1000, lib=emu_lib) == (forced, window_count(BN254, forced))
    with knobs(monkeypatch, width=21):   # (outside 2 .. 20: planned)
        assert ecc.batch_scalar_mul_plan("bn254", 1000, lib=emu_lib)[0] <= 18
    assert emu_lib.ga_batch_scalar_mul_plan(7, 10, None, None) == -1


def test_fixed_base_symbol_and_flags(emu_lib):
    """the entry point is exported and bound, and its two flags are the bits no other flag uses"""
    assert "ga_batch_scalar_mul" in _lib.EXPORTED_SYMBOLS and hasattr(emu_lib, "ga_batch_scalar_mul")
    assert (_lib.RESULT_ON_DEVICE, _lib.RESULT_BITREVERSED) == (0x20, 0x40)

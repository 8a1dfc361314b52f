"""kzg.ToLagrangeG1 on the device (ga_kzg_to_lagrange_g1, gnark_amd/csrc/ec_ntt.hip.h: the inverse FFT over G1 points that turns a
monomial SRS [tau^i]G1 into [l_i(tau)]G1) on the functional emulation.  Every case is a function of a context;
tests/test_to_lagrange_gpu.py runs the same cases on the device.  Every comparison is exact."""
import json
import os
import sys

import numpy as np
import pytest

import oracle
import pyref
import test_fixed_base as fb
from gnark_amd import _lib, ecc
from gnark_amd._lib import GnarkAmdError
from gnark_amd.device import affine_words
from helpers import BLS12_381, BN254, fr_to_arr, pts_to_arr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = [BN254, BLS12_381]
SIZES = (1, 2, 4, 8, 64, 128, 256, 1024)
ADICITY = {BN254.name: 28, BLS12_381.name: 32}


def tau_of(c):
    return pyref.Xoshiro(0x7A0 + c.cid).field(c.r)


def lagrange_scalars(c, n, tau, idx=None):
    """l_i(tau) = (tau^n - 1) w^i / (n (tau - w^i)) over the size-n domain (the formula of tests/test_gpu_parity.py's KZG case)"""
    w, ninv = c.fr_root_of_unity(n), pow(n, -1, c.r)
    tn1 = (pow(tau, n, c.r) - 1) % c.r
    out = []
    for i in (range(n) if idx is None else idx):
        wi = pow(w, i, c.r)
        out.append(tn1 * wi % c.r * ninv % c.r * pow((tau - wi) % c.r, -1, c.r) % c.r)
    return out


def powers_of(c, n, tau):
    ks, t = [], 1
    for _ in range(n):
        ks.append(t)
        t = t * tau % c.r
    return ks


def golden_srs():
    g = np.load(os.path.join(ROOT, "tests", "golden", "kzg4096_bls12381.npz"))
    return np.ascontiguousarray(g["g1_monomial"], dtype=np.uint64), np.ascontiguousarray(g["g1_lagrange"], dtype=np.uint64)


# ---- 1. known tau, point for point ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_to_lagrange_known_tau(emu_ctx, c, sizes=SIZES):
    """powers = [tau^i]G -> every output equals [l_i(tau)]G; n = 1 copies, n = 2 has only the 1/n twiddles, 64 butterflies fill one
    wave (n = 128), n = 1024 spans several workgroups, every stride and both lane orders"""
    tau = tau_of(c)
    for n in sizes:
        powers = fb.expected_points(c, 0, powers_of(c, n, tau))
        want = fb.expected_points(c, 0, lagrange_scalars(c, n, tau))
        got = ecc.ToLagrangeG1(emu_ctx, c.name, powers)
        assert got.shape == want.shape
        bad = np.where((got != want).any(axis=1))[0]
        assert bad.size == 0, (n, bad[:8])


# ---- 2. the ceremony golden ------------------------------------------------------------------------------------------------------
def test_to_lagrange_ceremony_golden(emu_ctx):
    """the EIP-4844 ceremony SRS (tau unknown): ToLagrangeG1(g1_monomial) == g1_lagrange, all 4096 points, byte for byte"""
    mono, lag = golden_srs()
    assert mono.shape == lag.shape == (4096, affine_words(BLS12_381.cid, 0))
    got = ecc.ToLagrangeG1(emu_ctx, BLS12_381.name, mono)
    bad = np.where((got != lag).any(axis=1))[0]
    assert bad.size == 0, bad[:8]


# ---- 3. degenerate inputs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 64, 256])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_to_lagrange_degenerate(emu_ctx, c, n):
    """all inputs the same point P (every butterfly a doubling and an a - b at infinity) -> out[0] = P, (0,0) elsewhere;
    tau = w (powers = [w^i]G) -> out[1] = G, (0,0) elsewhere"""
    wa = affine_words(c.cid, 0)
    P = fb.expected_points(c, 0, [0xC0FFEE])
    want = np.zeros((n, wa), np.uint64)
    want[0] = P[0]
    assert np.array_equal(ecc.ToLagrangeG1(emu_ctx, c.name, np.repeat(P, n, axis=0)), want)
    powers = fb.expected_points(c, 0, powers_of(c, n, c.fr_root_of_unity(n)))
    want = np.zeros((n, wa), np.uint64)
    want[1] = fb.gen_arr(c, 0)[0]
    assert np.array_equal(ecc.ToLagrangeG1(emu_ctx, c.name, powers), want)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_to_lagrange_random_points_with_infinities(emu_ctx, c, n=32):
    """32 unrelated points, three of them (0,0), against the definition out[i] = [1/n] sum_j [w^(-ij)] in[j] evaluated row by row
    with oracle.msm"""
    rng = pyref.Xoshiro(0x1A6 + c.cid)
    P = oracle.gen_bases(c.cid, 0, np.array([rng.next() for _ in range(n)], dtype=np.uint64)).copy()
    for j in (0, 13, 31):
        P[j] = 0
    winv, ninv = pow(c.fr_root_of_unity(n), -1, c.r), pow(n, -1, c.r)
    want = np.stack([oracle.jac_to_affine(c.cid, 0, oracle.msm(c.cid, 0, P, fr_to_arr(c, [pow(winv, i * j, c.r) * ninv % c.r for j in range(n)])))
                     for i in range(n)])
    assert np.array_equal(ecc.ToLagrangeG1(emu_ctx, c.name, P), want)


# ---- 4. placement and purity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_to_lagrange_placement_and_purity(emu_ctx, c, n=64):
    """host / device input x host / device output: equal bytes; the input buffer is byte-identical after the call, host and device"""
    ctx, wa = emu_ctx, affine_words(c.cid, 0)
    powers = fb.expected_points(c, 0, powers_of(c, n, tau_of(c)))
    want = fb.expected_points(c, 0, lagrange_scalars(c, n, tau_of(c)))
    keep = powers.copy()
    assert np.array_equal(ecc.ToLagrangeG1(ctx, c.name, powers), want) and np.array_equal(powers, keep)
    d_in = ctx.to_device(powers)
    try:
        assert np.array_equal(ecc.ToLagrangeG1(ctx, c.name, d_in, n=n), want)
        for src in (d_in, powers):
            d_out = ecc.ToLagrangeG1(ctx, c.name, src, n=n, out_device=True)
            try:
                assert np.array_equal(d_out.to_host((n, wa)), want)
            finally:
                d_out.free()
        assert np.array_equal(d_in.to_host((n, wa)), keep) and np.array_equal(powers, keep)
    finally:
        d_in.free()


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_to_lagrange_errors(emu_ctx, monkeypatch, c, n=16):
    """n = 3 and n = 1000: GA_ERR_INVALID and the next valid call succeeds; n = 0: GA_OK, nothing touched (include/gnark_amd.h; the
    same as every other entry point); n above 2^(two-adicity of r): rejected before anything is allocated or read; null pointers,
    an unknown curve; GA_FAULT_THROW: an error code, then the same call with the same result"""
    ctx, lib, h = emu_ctx, emu_ctx.lib, emu_ctx.handle
    wa = affine_words(c.cid, 0)
    powers = fb.expected_points(c, 0, powers_of(c, n, tau_of(c)))
    want = fb.expected_points(c, 0, lagrange_scalars(c, n, tau_of(c)))
    big = np.repeat(powers, 63, axis=0)[:1000].copy()
    out = np.full((1000, wa), 0xAB, np.uint64)
    P = lambda a: a.ctypes.data
    for bad_n in (3, 1000):
        assert lib.ga_kzg_to_lagrange_g1(h, c.cid, P(big), bad_n, 0, P(out)) == -1
        assert (out == 0xAB).all()
        assert np.array_equal(ecc.ToLagrangeG1(ctx, c.name, powers), want)
    with pytest.raises(GnarkAmdError):
        ecc.ToLagrangeG1(ctx, c.name, big)
    assert lib.ga_kzg_to_lagrange_g1(h, c.cid, None, 0, 0, None) == 0
    assert lib.ga_kzg_to_lagrange_g1(h, c.cid, P(big), 0, 0, P(out)) == 0 and (out == 0xAB).all()
    assert ecc.ToLagrangeG1(ctx, c.name, np.zeros((0, wa), np.uint64)).shape == (0, wa)
    # one step above the two-adicity: the 16-point buffers are all the memory there is behind the pointers
    assert lib.ga_kzg_to_lagrange_g1(h, c.cid, P(powers), 1 << (ADICITY[c.name] + 1), 0, P(out)) == -1 and (out == 0xAB).all()
    assert lib.ga_kzg_to_lagrange_g1(h, c.cid, P(powers), 1 << (ADICITY[c.name] + 1), _lib.BASES_ON_DEVICE | _lib.RESULT_ON_DEVICE, P(out)) == -1
    assert lib.ga_kzg_to_lagrange_g1(h, 7, P(powers), n, 0, P(out)) == -1
    assert lib.ga_kzg_to_lagrange_g1(h, c.cid, None, n, 0, P(out)) == -1
    assert lib.ga_kzg_to_lagrange_g1(h, c.cid, P(powers), n, 0, None) == -1
    assert lib.ga_kzg_to_lagrange_g1(None, c.cid, P(powers), n, 0, P(out)) == -1
    assert (out == 0xAB).all()
    try:
        monkeypatch.setenv("GA_FAULT_THROW", "ga_kzg_to_lagrange_g1")
        with pytest.raises(GnarkAmdError, match=r"error -3: out of host memory \(std::bad_alloc\) under ga_kzg_to_lagrange_g1"):
            ecc.ToLagrangeG1(ctx, c.name, powers)
        monkeypatch.delenv("GA_FAULT_THROW")
        assert np.array_equal(ecc.ToLagrangeG1(ctx, c.name, powers), want)
    finally:
        monkeypatch.delenv("GA_FAULT_THROW", raising=False)


def test_to_lagrange_lane_orders_agree(emu_ctx, monkeypatch, c=BN254, n=256):
    """GA_EC_NTT_UNIFORM=0 (consecutive butterflies of one group in a wave at every stage) gives the bytes of the default order"""
    powers = fb.expected_points(c, 0, powers_of(c, n, tau_of(c)))
    want = fb.expected_points(c, 0, lagrange_scalars(c, n, tau_of(c)))
    try:
        monkeypatch.setenv("GA_EC_NTT_UNIFORM", "0")
        assert np.array_equal(ecc.ToLagrangeG1(emu_ctx, c.name, powers), want)
    finally:
        monkeypatch.delenv("GA_EC_NTT_UNIFORM", raising=False)


# ---- 7. binding ------------------------------------------------------------------------------------------------------------------
def test_to_lagrange_symbol_and_go_binding(emu_lib):
    """the entry point is exported and bound; ga.go calls it and go/IDENTS.json resolves that call against the header"""
    assert "ga_kzg_to_lagrange_g1" in _lib.EXPORTED_SYMBOLS and hasattr(emu_lib, "ga_kzg_to_lagrange_g1")
    go = open(os.path.join(ROOT, "go", "backend", "accelerated", "mi355x", "internal", "ga", "ga.go")).read()
    assert "func (c *Context) ToLagrangeG1(" in go and "C.ga_kzg_to_lagrange_g1(c.h, C.int(curve), powers, C.size_t(n), C.uint(flags), outAffine)" in go
    idents = json.load(open(os.path.join(ROOT, "go", "IDENTS.json")))["resolved"]
    assert ["go/backend/accelerated/mi355x/internal/ga/ga.go", "C.ga_kzg_to_lagrange_g1", "include/gnark_amd.h prototype (6 args)"] in idents
    header = open(os.path.join(ROOT, "include", "gnark_amd.h")).read()
    assert "int ga_kzg_to_lagrange_g1(ga_ctx* ctx, int curve, const void* powers_affine, size_t n, unsigned flags, void* out_affine);" in header


# ---- the unreduced sequence of the butterfly ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", ["bn254", "bls12-381"])
def test_ladder_bounds(curve):
    """tools/lazy_bounds.py check_ladder: dbl29 and add29 alternating on each other's outputs, started from canonical and negated
    points, keep every value 2.5 bits below R' and satisfy every subtraction constant; the loop in ec_ntt.hip.h is made of exactly
    those two functions (whose constants tests/test_lazy_bounds.py ties to the analysis)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import lazy_bounds
    out = lazy_bounds.check_ladder(curve)
    assert all(v < out["limit"] - 2.5 for k, v in out.items() if k != "limit")
    src = open(os.path.join(ROOT, "gnark_amd", "csrc", "ec_ntt.hip.h")).read()
    body = src[src.index("__device__ __forceinline__ void ec_ntt_scalar_mul29("):src.index("__device__ __forceinline__ Lazy4<F> ec_ntt_unpack(")]
    assert "dbl29<F>(acc);" in body and "add29<F>(acc, d);" in body and "f29_" not in body
    stage = src[src.index("ec_ntt_stage_kernel("):src.index("// the flagged butterflies of a stage once more")]
    assert stage.count("f29_sub<2>(") == 1 and "f29_sub<" not in stage.replace("f29_sub<2>(", "")   # the negated y is the only other arithmetic

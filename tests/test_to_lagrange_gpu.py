"""ga_kzg_to_lagrange_g1 on a real MI355X: the cases of tests/test_to_lagrange.py through the hipcc-built library, and the chain the
entry point exists for at n = 2^16 -- powers of tau from ga_batch_scalar_mul, the Lagrange SRS from them, a pinned window table over
it -- without a point leaving the device."""
import numpy as np
import pytest

import oracle
import pyref
import test_fixed_base as fb
import test_to_lagrange as cases
from gnark_amd import ecc, fft
from gnark_amd.device import affine_words
from helpers import BLS12_381, BN254, fr_to_arr

pytestmark = pytest.mark.gpu
CURVES = [BN254, BLS12_381]


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_to_lagrange_known_tau(gpu_ctx, c):
    cases.test_to_lagrange_known_tau(gpu_ctx, c)


def test_to_lagrange_ceremony_golden(gpu_ctx):
    cases.test_to_lagrange_ceremony_golden(gpu_ctx)


@pytest.mark.parametrize("n", [16, 64, 256])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_to_lagrange_degenerate(gpu_ctx, c, n):
    cases.test_to_lagrange_degenerate(gpu_ctx, c, n)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_to_lagrange_random_points_with_infinities(gpu_ctx, c):
    cases.test_to_lagrange_random_points_with_infinities(gpu_ctx, c)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_to_lagrange_placement_and_purity(gpu_ctx, c):
    cases.test_to_lagrange_placement_and_purity(gpu_ctx, c)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_to_lagrange_errors(gpu_ctx, monkeypatch, c):
    cases.test_to_lagrange_errors(gpu_ctx, monkeypatch, c)


def test_to_lagrange_lane_orders_agree(gpu_ctx, monkeypatch):
    cases.test_to_lagrange_lane_orders_agree(gpu_ctx, monkeypatch, n=1024)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_to_lagrange_chain_2_16(gpu_ctx, c, logn=16):
    """n = 2^16: powers = ga_batch_scalar_mul over tau^i (device), Lagrange SRS = ga_kzg_to_lagrange_g1 of them (device), pinned with
    ga_msm_table_create as a device pointer.  For a random polynomial p:  table.MultiExp(evaluations of p, natural order) ==
    MultiExp(powers, p) == [p(tau)]G; 256 sampled outputs equal [l_i(tau)]G point for point; the powers are untouched"""
    ctx, n = gpu_ctx, 1 << logn
    wa = affine_words(c.cid, 0)
    tau = cases.tau_of(c)
    pw = cases.powers_of(c, n, tau)
    rng = pyref.Xoshiro(0xC4A1 + c.cid)
    p = [rng.field(c.r) for _ in range(n)]
    P = fr_to_arr(c, p)
    want = oracle.jac_to_affine(c.cid, 0, oracle.generator_mul(c.cid, 0, sum(a * b for a, b in zip(p, pw)) % c.r))
    d_pow = ecc.BatchScalarMultiplication(ctx, c.name, 0, fb.gen_arr(c, 0), fr_to_arr(c, pw, mont=False), out_device=True)
    d_lag = table = d = None
    try:
        before = d_pow.to_host((n, wa))
        d_lag = ecc.ToLagrangeG1(ctx, c.name, d_pow, n=n, out_device=True)
        assert np.array_equal(d_pow.to_host((n, wa)), before)
        table = ecc.PrecomputedBases(ctx, c.name, 0, d_lag, n=n)
        d = fft.Domain(ctx, c.name, n)
        ev = d.FFT(P, fft.DIF)   # bit-reversed evaluations
        idx = np.array([pyref.bitrev(i, logn) for i in range(n)])
        assert np.array_equal(oracle.jac_to_affine(c.cid, 0, table.MultiExp(ev[idx])), want)
        assert np.array_equal(oracle.jac_to_affine(c.cid, 0, ecc.MultiExp(ctx, c.name, 0, d_pow, P, n=n)), want)
        assert np.array_equal(oracle.jac_to_affine(c.cid, 0, ecc.MultiExp(ctx, c.name, 0, d_lag, ev[idx], n=n)), want)
        lag = d_lag.to_host((n, wa))
        sample = sorted({0, 1, n // 2, n - 1} | {rng.next() % n for _ in range(252)})
        assert np.array_equal(lag[sample], fb.expected_points(c, 0, cases.lagrange_scalars(c, n, tau, sample)))
    finally:
        if d is not None:
            d.close()
        if table is not None:
            table.free()
        for b in (d_lag, d_pow):
            if b is not None:
                b.free()

"""ga_scale_points on a real MI355X: the cases of tests/test_scale_points.py through the hipcc-built library, and the ceremony replay
at N = 2^12 with an MSM over the updated SRS, without a point leaving the device."""
import numpy as np
import pytest

import oracle
import pyref
import test_fixed_base as fb
import test_scale_points as cases
from gnark_amd import ecc
from gnark_amd.device import affine_words
from helpers import BLS12_381, BN254, fr_to_arr

pytestmark = pytest.mark.gpu
CURVES = [BN254, BLS12_381]


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_scale_points_modes(gpu_ctx, c, group, mode):
    cases.test_scale_points_modes(gpu_ctx, c, group, mode, sizes=cases.SIZES)


@pytest.mark.parametrize("mont", [False, True], ids=["canonical", "montgomery"])
@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_scale_points_edge_scalars(gpu_ctx, c, group, mont):
    cases.test_scale_points_edge_scalars(gpu_ctx, c, group, mont)


@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_scale_points_infinities_and_equal_points(gpu_ctx, c, group):
    cases.test_scale_points_infinities_and_equal_points(gpu_ctx, c, group)


def test_scale_points_order3_point(gpu_ctx):
    cases.test_scale_points_order3_point(gpu_ctx)


@pytest.mark.parametrize("c,group", [(BN254, 0), (BLS12_381, 0), (BN254, 1), (BLS12_381, 1)], ids=["bn254-G1", "bls12-381-G1", "bn254-G2", "bls12-381-G2"])
def test_scale_points_chunks_and_plain_ladder(gpu_ctx, monkeypatch, c, group):
    cases.test_scale_points_chunks_and_plain_ladder(gpu_ctx, monkeypatch, c, group)


@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_scale_points_placement_and_purity(gpu_ctx, monkeypatch, c, group):
    cases.test_scale_points_placement_and_purity(gpu_ctx, monkeypatch, c, group)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_scale_points_errors(gpu_ctx, monkeypatch, c):
    cases.test_scale_points_errors(gpu_ctx, monkeypatch, c)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_scale_points_ceremony_2_12(gpu_ctx, c, N=1 << 12):
    """N = 2^12: setOne, two SrsCommons.update steps and a phase-2 scaling in place on the device (64 sampled points of every vector
    against the oracle); then ga_msm over the updated G1.Tau[:N], still on the device, with random coefficients == [p(tau1 tau2)]G"""
    tau1, T = cases.ceremony_replay(gpu_ctx, c, N, check_all=False)
    try:
        rng = pyref.Xoshiro(0xC4A2 + c.cid)
        p = [rng.field(c.r) for _ in range(N)]
        want = oracle.jac_to_affine(c.cid, 0, oracle.generator_mul(c.cid, 0, sum(a * pow(T, i, c.r) for i, a in enumerate(p)) % c.r))
        assert np.array_equal(oracle.jac_to_affine(c.cid, 0, ecc.MultiExp(gpu_ctx, c.name, 0, tau1, fr_to_arr(c, p), n=N)), want)
    finally:
        tau1.free()


@pytest.mark.parametrize("c,group,n", [(BN254, 0, (1 << 18) + 77), (BLS12_381, 0, (1 << 18) + 77), (BLS12_381, 1, (1 << 17) + 77)],
                         ids=["bn254-G1", "bls12-381-G1", "bls12-381-G2"])
def test_scale_points_beyond_one_grid(gpu_ctx, monkeypatch, c, group, n):
    """more points than the 1024 workgroups of a ladder launch hold (256 lanes each, 128 for BLS12-381 G2): the grid-stride loop, both
    ladders.  Inputs [a_i]G from ga_batch_scalar_mul on the device; sum_i [z_i] out[i] == [sum z_i a_i s_i]G by ga_msm over the
    device-resident output, and the points on either side of the first stride and at the end against the oracle"""
    ctx, wa = gpu_ctx, affine_words(c.cid, group)
    rng = np.random.default_rng(0x617D + c.cid + group)

    def rand_words():
        w = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        w[:, 3] = rng.integers(1, c.r >> 192, size=n, dtype=np.uint64)   # below r
        return w, [int.from_bytes(row.tobytes(), "little") for row in w]
    (A, a), (S, s), (Z, z) = rand_words(), rand_words(), rand_words()
    stride = 1024 * (128 if (c, group) == (BLS12_381, 1) else 256)
    sample = [0, stride - 1, stride, stride + 1, n - 1]
    want_pts = fb.expected_points(c, group, [a[i] * s[i] % c.r for i in sample])
    want_sum = oracle.jac_to_affine(c.cid, group, oracle.generator_mul(c.cid, group, sum(x * y % c.r * w for x, y, w in zip(a, s, z)) % c.r))
    d_pts = ecc.BatchScalarMultiplication(ctx, c.name, group, fb.gen_arr(c, group), A, out_device=True)
    d_out = None
    try:
        for window in (None, 0):
            with cases.knobs(monkeypatch, window=window):
                d_out, redone = ecc.ScalePoints(ctx, c.name, group, d_pts, S, n=n, out_device=True)
            assert redone == 0
            assert np.array_equal(d_out.to_host((n, wa))[sample], want_pts), window
            assert np.array_equal(oracle.jac_to_affine(c.cid, group, ecc.MultiExp(ctx, c.name, group, d_out, Z, n=n, montgomery=False)), want_sum), window
            d_out.free()
            d_out = None
    finally:
        for b in (d_out, d_pts):
            if b is not None:
                b.free()

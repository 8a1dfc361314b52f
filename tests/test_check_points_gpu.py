"""ga_check_points and the checked key reads on a real MI355X: the cases of tests/test_check_points.py through the hipcc-built library,
and a vector longer than one grid of the ladder kernel."""
import numpy as np
import pytest

import pyref
import test_check_points as cases
import test_fixed_base as fb
from gnark_amd import ecc
from gnark_amd.device import affine_words
from helpers import BLS12_381, BN254, group_of, pts_to_arr

pytestmark = pytest.mark.gpu
CURVES = [BN254, BLS12_381]


@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_check_points_honest(gpu_ctx, c, group):
    cases.test_check_points_honest(gpu_ctx, c, group)


@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_check_points_mixed(gpu_ctx, c, group):
    cases.test_check_points_mixed(gpu_ctx, c, group)


@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_check_points_naive_and_chunks(gpu_ctx, monkeypatch, c, group):
    cases.test_check_points_naive_and_chunks(gpu_ctx, monkeypatch, c, group)


def test_check_points_order3_point(gpu_ctx, monkeypatch):
    cases.test_check_points_order3_point(gpu_ctx, monkeypatch)


@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_check_points_placement_and_purity(gpu_ctx, c, group):
    cases.test_check_points_placement_and_purity(gpu_ctx, c, group)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_check_points_errors(gpu_ctx, c):
    cases.test_check_points_errors(gpu_ctx, c)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_checked_key_reads(gpu_ctx, c):
    cases.test_checked_key_reads(gpu_ctx, c)


@pytest.mark.parametrize("c,group,n", [(BN254, 0, (1 << 18) + 77), (BLS12_381, 0, (1 << 18) + 77), (BLS12_381, 1, (1 << 17) + 77)],
                         ids=["bn254-G1", "bls12-381-G1", "bls12-381-G2"])
def test_check_points_beyond_one_grid(gpu_ctx, monkeypatch, c, group, n):
    """more points than the 1024 workgroups of a ladder launch hold (256 lanes each, 128 for BLS12-381 G2): the grid-stride loop, the
    fast test and the naive one.  Points [a_i]G from ga_batch_scalar_mul on the device, P + [r]Q planted on either side of the first
    grid stride and at n - 1 (on BN254 G1, where every curve point is in the group, y + 1 instead): counts and first exact, status
    exact at the sampled indices"""
    ctx, wa = gpu_ctx, affine_words(c.cid, group)
    G = group_of(c, group)
    rng = np.random.default_rng(0xC4EC + c.cid + group)
    A = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    A[:, 3] = rng.integers(1, c.r >> 192, size=n, dtype=np.uint64)   # below r, not zero
    stride = 1024 * (128 if (c, group) == (BLS12_381, 1) else 256)
    planted = [stride - 1, stride, n - 1]
    sample = [0, stride - 2, stride - 1, stride, stride + 1, n - 2, n - 1]
    prng = pyref.Xoshiro(0xBE70 + c.cid + group)
    kind = cases.OFF if (c, group) == (BN254, 0) else cases.OUT
    bad = []
    for i in planted:
        x, y = G.mul(cases.gen_of(c, group), int.from_bytes(A[i].tobytes(), "little"))
        if kind == cases.OFF:
            P = (x, (y + 1) % c.p)
        else:
            P = G.add((x, y), G.mul(cases.random_curve_point(c, group, prng), c.r))
        assert cases.model_status(c, group, P) == kind
        bad.append(pts_to_arr(c, group, [P])[0])
    d_pts = ecc.BatchScalarMultiplication(ctx, c.name, group, fb.gen_arr(c, group), A, out_device=True)
    try:
        host = d_pts.to_host((n, wa))
        for i, row in zip(planted, bad):
            host[i] = row
        d_bad = ctx.to_device(host)
        try:
            for naive in (None, 1):
                with cases.knobs(monkeypatch, naive=naive):
                    st, off, out, first, redone = ecc.CheckPoints(ctx, c.name, group, d_bad, n=n)
                want = (3, 0) if kind == cases.OFF else (0, 3)
                assert (off, out, first, redone) == want + (stride - 1, 0), naive
                assert [int(st[i]) for i in sample] == [kind if i in planted else cases.OK for i in sample], naive
                assert int(st.astype(np.uint64).sum()) == 3 * kind, naive
            st, off, out, first, redone = ecc.CheckPoints(ctx, c.name, group, d_pts, n=n)
            assert not st.any() and (off, out, first, redone) == (0, 0, cases.NONE_BAD, 0)
        finally:
            d_bad.free()
    finally:
        d_pts.free()

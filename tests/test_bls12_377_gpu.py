"""BLS12-377 (curve id 2), the G1 / Fr side, on the device: the cases of tests/bls12_377_cases.py against pyref at the sizes of the
emulation run (tests/test_bls12_377.py) and at those only the device reaches -- MSMs of 2^14 points and of the first size planned
with c = 11, transforms of 2^13 and 2^14 (an odd and an even log, more than one pass)."""
import pytest

import bls12_377_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [1, 7, 1 << 8, 1 << 14])
def test_msm(gpu_ctx, n):
    c, _ = cases.case_msm(gpu_ctx, n)
    if n == 1 << 14:
        assert c == 11   # 253 = 11 * 23: the top window of 24 holds the signed-digit carry alone


def test_msm_first_size_planned_with_c11(gpu_ctx):
    """ga_msm_plan answers c = 11 for 11265 <= n <= 20479 (one run; its upper sizes are test_msm[16384]'s side of 2^14)"""
    runs = cases.plan_c11_sizes(gpu_ctx.lib, 1 << 14)
    assert runs == [(11265, 1 << 14)]
    assert cases.case_msm(gpu_ctx, runs[0][0], seed=11)[0] == 11


@pytest.mark.parametrize("table_c", [11, 23])
def test_msm_table_width_dividing_253(gpu_ctx, monkeypatch, table_c):
    cases.case_msm_table_width(gpu_ctx, 1 << 8, table_c, monkeypatch)


def test_group_helpers_and_synthetic_inputs(gpu_ctx):
    cases.case_group_helpers(gpu_ctx.lib)
    cases.case_synthetic(gpu_ctx)


@pytest.mark.parametrize("n", [2, 8, 1 << 10, 1 << 13, 1 << 14])
def test_fft(gpu_ctx, n):
    cases.case_fft(gpu_ctx, n)


def test_fft_batch(gpu_ctx):
    cases.case_fft_batch(gpu_ctx)


def test_compute_h(gpu_ctx):
    cases.case_compute_h(gpu_ctx)


@pytest.mark.parametrize("nb_bsb", [0, 1])
@pytest.mark.parametrize("n", [16, 1 << 8])
def test_plonk_grand_product_and_quotient(gpu_ctx, n, nb_bsb):
    cases.case_plonk(gpu_ctx, n, nb_bsb)


def test_plonk_batches(gpu_ctx, monkeypatch):
    cases.case_plonk_batches(gpu_ctx, monkeypatch)


def test_kzg_open(gpu_ctx):
    cases.case_kzg_open(gpu_ctx)


def test_fr_vectors_and_hash(gpu_ctx):
    cases.case_fr_vectors(gpu_ctx)


def test_batch_scalar_mul(gpu_ctx):
    cases.case_batch_scalar_mul(gpu_ctx)


@pytest.mark.parametrize("n", [1 << 4, 1 << 8])
def test_to_lagrange_g1(gpu_ctx, n):
    cases.case_to_lagrange(gpu_ctx, n)


def test_check_points(gpu_ctx, monkeypatch):
    cases.case_check_points(gpu_ctx, monkeypatch)


def test_refusals(gpu_ctx):
    cases.case_refusals(gpu_ctx)

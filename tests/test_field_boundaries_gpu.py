"""The boundary-value cases of tests/field_cases.py on the device: the probe (tests/probe/field_probe.hip) as hipcc built it for gfx950
(gnark_amd/csrc/Makefile), so that what the compiler folded for the GPU -- kp_limb, mod_limb, the unrolled carry chains -- is what runs."""
import os

import pytest

import field_cases as fc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="session")
def gpu_probe():
    so = os.path.join(HERE, "probe", "libga_probe.so")
    if not os.path.exists(so):
        pytest.fail("tests/probe/libga_probe.so is missing: make -C gnark_amd/csrc builds it")
    return fc.Probe(so)


@pytest.mark.parametrize("field", sorted(fc.FIELDS))
@pytest.mark.parametrize("case", sorted(fc.FIELD_CASES))
def test_field_primitive(gpu_probe, case, field):
    fc.FIELD_CASES[case](gpu_probe, fc.FIELDS[field])


@pytest.mark.parametrize("field", fc.FP2_FIELDS)
@pytest.mark.parametrize("case", sorted(fc.BASE_FIELD_CASES))
def test_fp2_primitive(gpu_probe, case, field):
    fc.BASE_FIELD_CASES[case](gpu_probe, fc.FIELDS[field])


# (G2 only over a field that has an Fp2: not BLS12-377's)
@pytest.mark.parametrize("fp2,field", [pytest.param(fp2, n, id=("G2-" if fp2 else "G1-") + n) for n, fp2 in fc.POINT_FIELDS])
@pytest.mark.parametrize("case", sorted(fc.POINT_CASES))
def test_point_formula(gpu_probe, case, fp2, field):
    fc.POINT_CASES[case](gpu_probe, fc.FIELDS[field], fp2)


@pytest.mark.parametrize("c,cbits", fc.DIGIT_CASES, ids=lambda v: getattr(v, "name", str(v)))
def test_digit_recoding(gpu_probe, c, cbits):
    fc.case_digit_walk(gpu_probe, c, cbits)


# ---- boundary inputs through the shipped library on the device ----------------------------------------------------------------
@pytest.mark.parametrize("c", fc.CURVES, ids=lambda c: c.name)
def test_msm_crafted_raw(gpu_ctx, c, monkeypatch):
    fc.case_msm_crafted(gpu_ctx, c, fc.planned_width(gpu_ctx, c), False, monkeypatch.setenv)


@pytest.mark.parametrize("c,cbits", fc.TABLE_CASES, ids=lambda v: getattr(v, "name", str(v)))
def test_msm_crafted_table(gpu_ctx, c, cbits, monkeypatch):
    fc.case_msm_crafted(gpu_ctx, c, cbits, True, monkeypatch.setenv)


@pytest.mark.parametrize("c", fc.CURVES, ids=lambda c: c.name)
def test_fr_vector_ops(gpu_ctx, c):
    fc.case_fr_vector_ops(gpu_ctx, c)


@pytest.mark.parametrize("c", fc.CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("logn", fc.FFT_LOGN)
def test_fft_boundary_inputs(gpu_ctx, c, logn):
    fc.case_fft_boundary_inputs(gpu_ctx, c, logn)


@pytest.mark.parametrize("c", fc.CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("n", [8, 64])
def test_plonk_constant_inputs(gpu_ctx, c, n):
    fc.case_plonk_constant_inputs(gpu_ctx, c, n)


@pytest.mark.parametrize("c", fc.CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("knobs", sorted(fc.FFT_2P17_KNOBS))
def test_fft_boundary_inputs_2p17(gpu_ctx, monkeypatch, knobs, c):
    for k, v in fc.FFT_2P17_KNOBS[knobs].items():
        monkeypatch.setenv(k, v)
    fc.case_fft_boundary_inputs(gpu_ctx, c, 17)

"""Boundary values through the device primitives of the field layer and the point formulas on it, under the functional emulation:
the probe (tests/probe/field_probe.hip) compiled by g++ against tests/emu/include.  The cases are tests/field_cases.py; the same cases
run on the device in tests/test_field_boundaries_gpu.py."""
import os
import subprocess

import pytest

import field_cases as fc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="session")
def emu_probe():
    so = os.path.join(HERE, "probe", "libga_probe_emu.so")
    r = subprocess.run([os.path.join(HERE, "probe", "build_probe_emu.sh")], capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(so):
        pytest.fail("emulation build of the probe failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
    return fc.Probe(so)


@pytest.mark.parametrize("field", sorted(fc.FIELDS))
@pytest.mark.parametrize("case", sorted(fc.FIELD_CASES))
def test_field_primitive(emu_probe, case, field):
    fc.FIELD_CASES[case](emu_probe, fc.FIELDS[field])


@pytest.mark.parametrize("field", fc.FP2_FIELDS)
@pytest.mark.parametrize("case", sorted(fc.BASE_FIELD_CASES))
def test_fp2_primitive(emu_probe, case, field):
    fc.BASE_FIELD_CASES[case](emu_probe, fc.FIELDS[field])


# (G2 only over a field that has an Fp2: not BLS12-377's)
@pytest.mark.parametrize("fp2,field", [pytest.param(fp2, n, id=("G2-" if fp2 else "G1-") + n) for n, fp2 in fc.POINT_FIELDS])
@pytest.mark.parametrize("case", sorted(fc.POINT_CASES))
def test_point_formula(emu_probe, case, fp2, field):
    fc.POINT_CASES[case](emu_probe, fc.FIELDS[field], fp2)


def test_probe_refuses_bad_arguments(emu_probe):
    """a word count that is not the op's, an unknown op, field or template constant: refused before anything is launched"""
    import ctypes
    buf = (ctypes.c_uint32 * 64)()
    f = emu_probe.fn
    assert f(0, fc.OP_ADD, 0, buf, 1, 15, buf, 8) == 1
    assert f(0, fc.OP_ADD, 0, buf, 1, 16, buf, 9) == 1
    assert f(0, 99, 0, buf, 1, 16, buf, 8) == 1
    assert f(7, fc.OP_ADD, 0, buf, 1, 16, buf, 8) == 1
    assert f(0, fc.OP_F29_SUB, 3, buf, 1, 18, buf, 9) == 1
    assert f(1, fc.OP_F29X2_MUL, 0, buf, 1, 36, buf, 18) == 1     # Fp2 over a scalar field
    assert f(0, fc.OP_PT_ADD29, 65, buf, 0, 72, buf, 36) == 1     # chain longer than the probe allows
    assert f(0, fc.OP_ADD, 0, buf, 1, 16, buf, 8) == 0
    # BLS12-377 Fp (field 4: 12 words, 14 limbs) has the G1 point formulas and no Fp2: the Fp2 ops, the point formulas over Fp2 and
    # the Fp2 negation constant of f29_mul_sub are refused, with the word counts they would have; n = 0 launches nothing either way
    assert f(4, fc.OP_F29X2_MUL, 0, buf, 0, 56, buf, 28) == 1
    assert f(4, fc.OP_PT_ADD29 + fc.OP_PT2, 1, buf, 0, 224, buf, 112) == 1
    assert f(4, fc.OP_F29_MUL_SUB, fc.FP2Z_K, buf, 0, 56, buf, 14) == 1
    assert f(4, fc.OP_F29_MUL_SUB, 8, buf, 0, 56, buf, 14) == 0
    assert f(4, fc.OP_PT_ADD29, 1, buf, 0, 112, buf, 56) == 0
    assert f(2, fc.OP_PT_ADD29 + fc.OP_PT2, 1, buf, 0, 224, buf, 112) == 0


@pytest.mark.parametrize("c,cbits", fc.DIGIT_CASES, ids=lambda v: getattr(v, "name", str(v)))
def test_digit_recoding(emu_probe, c, cbits):
    fc.case_digit_walk(emu_probe, c, cbits)


# ---- boundary inputs through the shipped library under the emulation ------------------------------------------------------------
@pytest.mark.parametrize("c", fc.CURVES, ids=lambda c: c.name)
def test_msm_crafted_raw(emu_ctx, c, monkeypatch):
    fc.case_msm_crafted(emu_ctx, c, fc.planned_width(emu_ctx, c), False, monkeypatch.setenv)


@pytest.mark.parametrize("c,cbits", fc.TABLE_CASES, ids=lambda v: getattr(v, "name", str(v)))
def test_msm_crafted_table(emu_ctx, c, cbits, monkeypatch):
    fc.case_msm_crafted(emu_ctx, c, cbits, True, monkeypatch.setenv)


@pytest.mark.parametrize("c", fc.CURVES, ids=lambda c: c.name)
def test_fr_vector_ops(emu_ctx, c):
    fc.case_fr_vector_ops(emu_ctx, c)


@pytest.mark.parametrize("c", fc.CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("logn", fc.FFT_LOGN)
def test_fft_boundary_inputs(emu_ctx, c, logn):
    fc.case_fft_boundary_inputs(emu_ctx, c, logn)


@pytest.mark.parametrize("c", fc.CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("n", [8, 64])
def test_plonk_constant_inputs(emu_ctx, c, n):
    fc.case_plonk_constant_inputs(emu_ctx, c, n)


@pytest.mark.parametrize("c", fc.CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("knobs", sorted(fc.FFT_2P17_KNOBS))
def test_fft_boundary_inputs_2p17(emu_ctx, monkeypatch, knobs, c):
    """2^17: the size at which the transform splits into rounds, under every knob set that changes the split"""
    for k, v in fc.FFT_2P17_KNOBS[knobs].items():
        monkeypatch.setenv(k, v)
    fc.case_fft_boundary_inputs(emu_ctx, c, 17)

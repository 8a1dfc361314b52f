"""The point codec's verdicts and the multi-pass key streams on the functional emulation: the cases of tests/codec_cases.py (the strict
reference, the encoding table, the host and the device route, GA_KEY_CHUNK).  tests/test_codec_gpu.py runs them on the device."""
import pytest

import codec_cases as cases

CURVES = cases.CURVES
curve = pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
group = pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
mode = pytest.mark.parametrize("compressed", [True, False], ids=["compressed", "raw"])
knob = pytest.mark.parametrize("knob", cases.KNOBS, ids=lambda k: "chunk-%s" % k)


@mode
@group
@curve
def test_reference_agrees_with_construction(c, group, compressed):
    cases.test_reference_agrees_with_construction(c, group, compressed)


@mode
@group
@curve
def test_host_point_route(emu_lib, c, group, compressed):
    cases.test_host_point_route(emu_lib, c, group, compressed)


@mode
@group
@curve
def test_host_proof_route(emu_lib, c, group, compressed):
    cases.test_host_proof_route(emu_lib, c, group, compressed)


@mode
@curve
def test_device_route(emu_ctx, c, compressed):
    cases.test_device_route(emu_ctx, c, compressed)


@curve
def test_encode_thresholds_host(emu_lib, c):
    cases.test_encode_thresholds_host(emu_lib, c)


@curve
def test_encode_thresholds_device(emu_ctx, c):
    cases.test_encode_thresholds_device(emu_ctx, c)


@knob
@curve
def test_multipass_read_write(emu_ctx, monkeypatch, c, knob, tmp_path):
    cases.test_multipass_read_write(emu_ctx, monkeypatch, c, knob, tmp_path)


@knob
@curve
def test_multipass_shards(emu_ctx, monkeypatch, c, knob):
    cases.test_multipass_shards(emu_ctx, monkeypatch, c, knob)


@knob
@curve
def test_multipass_checked_reads(emu_ctx, monkeypatch, c, knob):
    cases.test_multipass_checked_reads(emu_ctx, monkeypatch, c, knob)


@knob
@curve
def test_multipass_undecodable_and_truncation(emu_ctx, monkeypatch, c, knob):
    cases.test_multipass_undecodable_and_truncation(emu_ctx, monkeypatch, c, knob)

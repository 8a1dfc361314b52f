"""The point codec's verdicts and the multi-pass key streams on a real MI355X: the cases of tests/codec_cases.py through the hipcc-built
library -- the host route (the codec compiled for the host by hipcc), the device route (key_decode_kernel / key_encode_kernel) and the
staging loops under GA_KEY_CHUNK.  The reference and the table are checked against each other in tests/test_codec.py."""
import pytest

import codec_cases as cases

pytestmark = pytest.mark.gpu

CURVES = cases.CURVES
curve = pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
group = pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
mode = pytest.mark.parametrize("compressed", [True, False], ids=["compressed", "raw"])
knob = pytest.mark.parametrize("knob", cases.KNOBS, ids=lambda k: "chunk-%s" % k)


@mode
@group
@curve
def test_host_point_route(gpu_ctx, c, group, compressed):
    cases.test_host_point_route(gpu_ctx.lib, c, group, compressed)


@mode
@group
@curve
def test_host_proof_route(gpu_ctx, c, group, compressed):
    cases.test_host_proof_route(gpu_ctx.lib, c, group, compressed)


@mode
@curve
def test_device_route(gpu_ctx, c, compressed):
    cases.test_device_route(gpu_ctx, c, compressed)


@curve
def test_encode_thresholds_host(gpu_ctx, c):
    cases.test_encode_thresholds_host(gpu_ctx.lib, c)


@curve
def test_encode_thresholds_device(gpu_ctx, c):
    cases.test_encode_thresholds_device(gpu_ctx, c)


@knob
@curve
def test_multipass_read_write(gpu_ctx, monkeypatch, c, knob, tmp_path):
    cases.test_multipass_read_write(gpu_ctx, monkeypatch, c, knob, tmp_path)


@knob
@curve
def test_multipass_shards(gpu_ctx, monkeypatch, c, knob):
    cases.test_multipass_shards(gpu_ctx, monkeypatch, c, knob)


@knob
@curve
def test_multipass_checked_reads(gpu_ctx, monkeypatch, c, knob):
    cases.test_multipass_checked_reads(gpu_ctx, monkeypatch, c, knob)


@knob
@curve
def test_multipass_undecodable_and_truncation(gpu_ctx, monkeypatch, c, knob):
    cases.test_multipass_undecodable_and_truncation(gpu_ctx, monkeypatch, c, knob)

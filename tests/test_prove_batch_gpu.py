"""ga_fft_batch, ga_compute_h_batch and ga_g16_prove_batch on a real MI355X: the cases of tests/test_prove_batch.py through the
hipcc-built library at the device sizes -- transforms of two and three passes and of many tiles per vector, sixteen vectors of one
tile, proofs at 2^10 and 2^11, seventeen proofs in chunks of 16 + 1."""
import numpy as np
import pytest

import test_prove_batch as cases
from helpers import BLS12_381, BN254

pytestmark = pytest.mark.gpu
CURVES = [BN254, BLS12_381]


@pytest.mark.parametrize("logn,count", [(3, 3), (9, 3), (10, 16), (11, 3), (13, 3), (16, 3)], ids=lambda v: str(v))
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_fft_batch_all_modes(gpu_ctx, c, logn, count):
    """a tile smaller than the workgroup's 1024 slots (2^3, 2^9), sixteen vectors of exactly one tile (2^10: sixteen workgroups in one
    launch), two passes (2^11, 2^13), three passes and 64 tiles per vector (2^16)"""
    cases.test_fft_batch_all_modes(gpu_ctx, c, logn, count)


@pytest.mark.parametrize("logn", [3, 10, 13])
def test_fft_batch_containment(gpu_ctx, logn):
    cases.test_fft_batch_containment(gpu_ctx, logn)


@pytest.mark.parametrize("c,plan", cases.FORCED_PLAN_CASES, ids=lambda v: getattr(v, "name", v))
def test_fft_batch_forced_plans(gpu_ctx, monkeypatch, c, plan):
    cases.test_fft_batch_forced_plans(gpu_ctx, monkeypatch, c, plan)


@pytest.mark.parametrize("plan,knobs", cases.FORCED_PLAN_KNOB_CASES)
def test_fft_batch_forced_plans_knobs(gpu_ctx, monkeypatch, plan, knobs):
    cases.test_fft_batch_forced_plans_knobs(gpu_ctx, monkeypatch, plan, knobs)


@pytest.mark.parametrize("short", [5, 0], ids=["n-5", "n"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_compute_h_batch(gpu_ctx, c, short):
    cases.test_compute_h_batch(gpu_ctx, c, short, logn=11)


def test_fft_batch_errors(gpu_ctx):
    cases.test_fft_batch_errors(gpu_ctx)


@pytest.mark.parametrize("kind", list(cases.KEY_KINDS))
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_prove_batch_layouts(gpu_ctx, monkeypatch, c, kind):
    cases.test_prove_batch_layouts(gpu_ctx, monkeypatch, c, kind, logn=10)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_prove_batch_chunks(gpu_ctx, monkeypatch, c):
    cases.test_prove_batch_chunks(gpu_ctx, monkeypatch, c, logn=10)


def test_prove_batch_seventeen(gpu_ctx, monkeypatch, c=BN254, logn=10, count=17):
    """the default chunk limit: seventeen solutions go through the device as 16 + 1"""
    ctx = gpu_ctx
    monkeypatch.delenv("GA_G16_BATCH_MAX", raising=False)
    want = cases.oracle_proofs(ctx, c, logn, "dense", count)
    pk = cases.pin(ctx, c, logn, "dense")
    try:
        cases.check_layout(pk, "dense")
        cases.assert_proofs(cases.prove_batch(pk, cases.solutions(ctx, c, logn, count)), want, "16 + 1")
    finally:
        pk.FreeGPUResources()


def test_prove_batch_two_pass_transforms(gpu_ctx, monkeypatch):
    """2^11: every transform of the batch's H side is two launches over the three vectors"""
    cases.test_prove_batch_layouts(gpu_ctx, monkeypatch, BN254, "dense", logn=11)


@pytest.mark.parametrize("precompute", [1, -1], ids=["tables", "no-tables"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_prove_batch_cubic(gpu_ctx, c, precompute):
    cases.test_prove_batch_cubic(gpu_ctx, c, precompute)


@pytest.mark.parametrize("precompute", [1, -1], ids=["tables", "no-tables"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_prove_batch_bsb22(gpu_ctx, c, precompute):
    cases.test_prove_batch_bsb22(gpu_ctx, c, precompute)


def test_prove_batch_refusals(gpu_ctx):
    cases.test_prove_batch_refusals(gpu_ctx, logn=10)


def test_prove_batch_exception_barrier(gpu_ctx, monkeypatch):
    cases.test_prove_batch_exception_barrier(gpu_ctx, monkeypatch, logn=10)


def test_prove_batch_beside_single_proof(gpu_ctx):
    cases.test_prove_batch_beside_single_proof(gpu_ctx, logn=6)

"""The cases of tests/test_abi_drivers.py on a real MI355X through the hipcc-built library: proofs over plain vectors at 2^10
constraints in chunks of 300 points (300 + 300 + 300 + a ragged rest), the single / batched pairs at 2^11."""
import pytest

import test_abi_drivers as cases
from helpers import BLS12_381, BN254

pytestmark = pytest.mark.gpu
CURVES = [BN254, BLS12_381]


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_prover_chunks(gpu_ctx, monkeypatch, c):
    cases.case_prover_chunks(gpu_ctx, monkeypatch, c, 10, 300)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_commit_chunks(gpu_ctx, monkeypatch, c):
    cases.case_commit_chunks(gpu_ctx, monkeypatch, c, 10, 300)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_fft_single_is_batch(gpu_ctx, c):
    cases.case_fft_single_is_batch(gpu_ctx, c, 11)


@pytest.mark.parametrize("short", [5, 0], ids=["n-5", "n"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_compute_h_single_is_batch(gpu_ctx, c, short):
    cases.case_compute_h_single_is_batch(gpu_ctx, c, 11, short)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_kzg_single_is_batch(gpu_ctx, monkeypatch, c):
    monkeypatch.delenv("GA_PLONK_BATCH_MAX", raising=False)
    cases.case_kzg_single_is_batch(gpu_ctx, c, 1 << 11)


@pytest.mark.parametrize("c,group", [(BN254, 0), (BN254, 1), (BLS12_381, 0)], ids=["bn254-g1", "bn254-g2", "bls12-381-g1"])
def test_table_run_shapes(gpu_ctx, c, group):
    cases.case_table_run_shapes(gpu_ctx, c, group, 1 << 11)


def test_refusal_names(gpu_ctx):
    cases.case_refusal_names(gpu_ctx)


def test_g16_refusal_names(gpu_ctx):
    cases.case_g16_refusal_names(gpu_ctx)


@pytest.mark.parametrize("short", [0, 3], ids=["n", "n-3"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_h_chain_dev_is_h_chain(gpu_ctx, c, short):
    cases.case_h_chain_dev_is_h_chain(gpu_ctx, c, 3, short)

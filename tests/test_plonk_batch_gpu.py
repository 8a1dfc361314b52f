"""ga_plonk_build_z_batch, ga_plonk_quotient_pinned_batch and ga_kzg_open_batch on a real MI355X: the case functions of
tests/test_plonk_batch.py through the hipcc-built library, at the smallest sizes where the device shapes differ from the emulation's
-- 2^10 (one NTT tile per vector, the segmented scans at their designed width), 2^11 (two transform passes), 2^13; three, sixteen
and seventeen (16 + 1) proofs; opening lengths 2^10 + 3 and 2^13 + 2 (the second needs a third entry of the upper power table).  The
single calls, the one-proof case of the same drivers, run against the oracles at the shapes of their emulation twins."""
import pytest

import test_plonk_batch as cases
from helpers import BLS12_381, BN254

pytestmark = pytest.mark.gpu
CURVES = [BN254, BLS12_381]


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    monkeypatch.delenv("GA_PLONK_BATCH_MAX", raising=False)
    monkeypatch.delenv("GA_PLONK_SCAN_THREADS", raising=False)


@pytest.mark.parametrize("logn,count", [(10, 16), (11, 3), (13, 3), (10, 17)], ids=lambda v: str(v))
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_build_z_batch(gpu_ctx, c, logn, count):
    cases.case_build_z(gpu_ctx, c, 1 << logn, count)


@pytest.mark.parametrize("logn,nb_bsb,count,lagrange", [(10, 1, 16, True), (10, 0, 3, False), (11, 1, 3, True), (13, 1, 3, True), (10, 1, 17, False)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_quotient_batch(gpu_ctx, c, logn, nb_bsb, count, lagrange):
    cases.case_quotient(gpu_ctx, c, 1 << logn, nb_bsb, count, lagrange)


@pytest.mark.parametrize("length,count", [((1 << 10) + 3, 16), ((1 << 13) + 2, 3), ((1 << 10) + 3, 17)], ids=lambda v: str(v))
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_open_batch(gpu_ctx, c, length, count):
    cases.case_open(gpu_ctx, c, length, length + 5, count)


def test_build_z_batch_on_device(gpu_ctx):
    cases.case_build_z(gpu_ctx, BN254, 1 << 10, 3, on_device=True)


def test_quotient_batch_on_device(gpu_ctx):
    cases.case_quotient(gpu_ctx, BN254, 1 << 10, 1, 3, True, on_device=True)


def test_open_batch_on_device(gpu_ctx):
    cases.case_open(gpu_ctx, BN254, (1 << 10) + 3, (1 << 10) + 8, 3, on_device=True)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_chunks(gpu_ctx, monkeypatch, c):
    """five proofs of 2^10 as 2 + 2 + 1"""
    cases.case_chunks(gpu_ctx, monkeypatch, c, 1 << 10, (1 << 10) + 3, 5, 2)


def test_build_z_uneven_passes(gpu_ctx, monkeypatch):
    """seventeen proofs of 2^13 in passes of nine and eight: at the default scan width nine proofs take prefix-product chunks of 16
    elements and eight on their own would take 8 -- twice the chunk products of the first pass; the chunk stays that of the first"""
    monkeypatch.setenv("GA_PLONK_BATCH_MAX", "9")
    cases.case_build_z(gpu_ctx, BN254, 1 << 13, 17)


def test_quotient_batch_mixed_mask(gpu_ctx):
    cases.case_quotient(gpu_ctx, BN254, 1 << 10, 1, 3, "mixed")


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_single_build_z_one_scan_thread(gpu_ctx, monkeypatch, c):
    """ga_plonk_build_z at n = 512 with GA_PLONK_SCAN_THREADS = 1: two chunks of 256"""
    monkeypatch.setenv("GA_PLONK_SCAN_THREADS", "1")
    cases.case_single_build_z(gpu_ctx, c, 512)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_single_open_above_one_table_block(gpu_ctx, c):
    """ga_kzg_open and ga_fr_poly_evaluate at 2^12 + 3 coefficients, at a random point and at the point 0"""
    cases.case_single_open(gpu_ctx, c, (1 << 12) + 3)


@pytest.mark.parametrize("n,nb_bsb", [(4, 0), (4, 1), (8, 0), (8, 1)])
def test_single_quotient_mixed_mask(gpu_ctx, n, nb_bsb):
    """ga_plonk_quotient_pinned at n = 4 (where |domain1| = 8 n) and n = 8 (the smallest size with rho = 4), a mixed Lagrange mask"""
    cases.case_single_quotient(gpu_ctx, BN254, n, nb_bsb)


def test_refusals(gpu_ctx):
    cases.case_refusals(gpu_ctx)


def test_exception_barrier(gpu_ctx, monkeypatch):
    cases.case_exception_barrier(gpu_ctx, monkeypatch)

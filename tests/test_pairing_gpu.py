"""ga_pairing_check and the Groth16 verifier on a real MI355X: the cases of tests/test_pairing.py through the hipcc-built library, and
a vector longer than one launch of the Miller kernel."""
import numpy as np
import pytest

import test_fixed_base as fb
import test_pairing as cases
from gnark_amd import ecc
from gnark_amd.device import affine_words
from helpers import BLS12_381, BN254

pytestmark = pytest.mark.gpu
CURVES = [BN254, BLS12_381]


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_pairing_against_oracle(gpu_ctx, c):
    cases.test_pairing_against_oracle(gpu_ctx, c)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_pairing_edges(gpu_ctx, monkeypatch, c):
    cases.test_pairing_edges(gpu_ctx, monkeypatch, c)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_pairing_infinity_and_purity(gpu_ctx, c):
    cases.test_pairing_infinity_and_purity(gpu_ctx, c)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_pairing_gt(gpu_ctx, c):
    cases.test_pairing_gt(gpu_ctx, c)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_pairing_errors(gpu_ctx, c):
    cases.test_pairing_errors(gpu_ctx, c)


def test_verify_bellman_tuples(gpu_ctx):
    cases.test_verify_bellman_tuples(gpu_ctx)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_verify_oracle_proofs_and_tampering(gpu_ctx, c):
    cases.test_verify_oracle_proofs_and_tampering(gpu_ctx, c)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_verify_many(gpu_ctx, c):
    cases.test_verify_many(gpu_ctx, c)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_batch_verify(gpu_ctx, c):
    cases.test_batch_verify(gpu_ctx, c)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_pairing_beyond_one_launch(gpu_ctx, c):
    """more pairs than the 1024 one-wave workgroups of a Miller launch hold (2^16 lanes): the grid-stride loop, and a group of 2^16
    pairs through four levels of partial products.  Points [a_i]G1, [b_i]G2 from ga_batch_scalar_mul on the device; group 0 is the
    first 77 pairs (not 1), group 1 the rest, closed by its last pair (-[sum a_i b_i]G1, G2).  Moving the closing pair into group 0
    flips group 1's verdict"""
    ctx = gpu_ctx
    n = 1024 * 64 + 77
    w1, w2 = affine_words(c.cid, 0), affine_words(c.cid, 1)
    rng = np.random.default_rng(0x9A12 + c.cid)

    def rand_words():   # scalars below r: the top word below r's
        w = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        w[:, 3] = rng.integers(1, c.r >> 192, size=n, dtype=np.uint64)
        return w
    A, B = rand_words(), rand_words()
    ints = lambda W: [int.from_bytes(row.tobytes(), "little") for row in W]
    a, b = ints(A), ints(B)
    ca, cb = cases.closing(c, a[77:n - 1], b[77:n - 1])
    dP = ecc.BatchScalarMultiplication(ctx, c.name, 0, fb.gen_arr(c, 0), A, out_device=True)
    dQ = ecc.BatchScalarMultiplication(ctx, c.name, 1, fb.gen_arr(c, 1), B, out_device=True)
    try:
        P, Q = dP.to_host((n, w1)), dQ.to_host((n, w2))
    finally:
        dP.free()
        dQ.free()
    P[n - 1], Q[n - 1] = fb.expected_points(c, 0, [ca])[0], fb.expected_points(c, 1, [cb])[0]
    gs = [0, 77, n]
    dP, dQ = ctx.to_device(P), ctx.to_device(Q)
    try:
        ok, bad, first = ecc.PairingCheck(ctx, c.name, dP, dQ, gs)
        assert list(ok) == [0, 1] and (bad, first) == (1, 0)
    finally:
        dP.free()
        dQ.free()
    P[[0, n - 1]] = P[[n - 1, 0]]
    Q[[0, n - 1]] = Q[[n - 1, 0]]
    dP, dQ = ctx.to_device(P), ctx.to_device(Q)
    try:
        ok, bad, first = ecc.PairingCheck(ctx, c.name, dP, dQ, gs)
        assert list(ok) == [0, 0] and (bad, first) == (2, 0)
    finally:
        dP.free()
        dQ.free()

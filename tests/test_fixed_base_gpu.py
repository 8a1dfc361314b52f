"""ga_batch_scalar_mul on a real MI355X: the cases of tests/test_fixed_base.py through the hipcc-built library, the default
window width at n = 2^16 point for point, and n = 2^18 by the known-discrete-log identity turned round."""
import numpy as np
import pytest

import oracle
import test_fixed_base as cases
from gnark_amd import ecc
from gnark_amd.device import affine_words
from helpers import BLS12_381, BN254

pytestmark = pytest.mark.gpu
CURVES = [BN254, BLS12_381]


@pytest.mark.parametrize("width", cases.WIDTHS + (None,), ids=["c4", "c7", "c13", "planned"])
@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_fixed_base_vs_oracle(gpu_ctx, monkeypatch, c, group, width):
    cases.test_fixed_base_vs_oracle(gpu_ctx, monkeypatch, c, group, width)


@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_fixed_base_planned_width_2_16(gpu_ctx, monkeypatch, c, group):
    """the planned window width at n = 2^16 (256 workgroups of the accumulation kernel, the lane batches of stage 3 across
    several waves): every one of the 65536 points equals the oracle's.  The expected points are 65536 calls of oracle.generator_mul +
    oracle.jac_to_affine on a pool of host threads, which is what a case waits for: 4.9 - 6.6 s per case measured, the device work included"""
    cases.test_fixed_base_vs_oracle(gpu_ctx, monkeypatch, c, group, None, sizes=(1 << 16,))


@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_fixed_base_other_bases(gpu_ctx, monkeypatch, c, group):
    cases.test_fixed_base_other_bases(gpu_ctx, monkeypatch, c, group)


@pytest.mark.parametrize("exact", [False, True], ids=["complete-lazy", "exact-kernel"])
def test_fixed_base_order3_base(gpu_ctx, monkeypatch, exact):
    cases.test_fixed_base_order3_base(gpu_ctx, monkeypatch, exact)


@pytest.mark.parametrize("c,group", [(BN254, 0), (BLS12_381, 1)], ids=["bn254-G1", "bls12-381-G2"])
def test_fixed_base_chunks_and_bitreversal(gpu_ctx, monkeypatch, c, group):
    cases.test_fixed_base_chunks_and_bitreversal(gpu_ctx, monkeypatch, c, group)


@pytest.mark.parametrize("circuit", ["cubic", "commit"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_fixed_base_reproduces_groth16_key(gpu_ctx, c, circuit):
    cases.test_fixed_base_reproduces_groth16_key(gpu_ctx, c, circuit)


@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
def test_fixed_base_2_18_known_dlog(gpu_ctx, group):
    """n = 2^18, BN254: with a second random vector t, MSM(out, t) == [sum t_i s_i] base -- the known-discrete-log check of the
    MSM tests turned round (the outputs are the bases, the scalars their discrete logs)"""
    ctx, lib, c, n = gpu_ctx, gpu_ctx.lib, BN254, 1 << 18
    s, t = ctx.malloc(n * 32), ctx.malloc(n * 32)
    out = None
    try:
        lib.check(lib.ga_gen_scalars(ctx.handle, c.cid, 0xF1B + group, n, s.ptr))
        lib.check(lib.ga_gen_scalars(ctx.handle, c.cid, 0xF1C + group, n, t.ptr))
        # s as canonical integers (gnark's setup passes them so): the image ga_gen_scalars wrote, read as an integer below r
        out = ecc.BatchScalarMultiplication(ctx, c.name, group, cases.gen_arr(c, group), s, n=n, out_device=True)
        got = oracle.jac_to_affine(c.cid, group, ecc.MultiExp(ctx, c.name, group, out, t, n=n))
        dot = np.zeros(4, dtype=np.uint64)
        lib.check(lib.ga_fr_dot(ctx.handle, c.cid, t.ptr, s.ptr, n, dot.ctypes.data))   # t Montgomery, s canonical -> canonical
        k = sum(int(v) << (64 * i) for i, v in enumerate(dot))
        assert k == oracle.fr_dot(c.cid, t.to_host((n, 4)), s.to_host((n, 4)))
        assert got.any() and np.array_equal(got, oracle.jac_to_affine(c.cid, group, oracle.generator_mul(c.cid, group, k)))
        assert out.nbytes == n * affine_words(c.cid, group) * 8
    finally:
        for b in (s, t, out):
            if b is not None:
                b.free()

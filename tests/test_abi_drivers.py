"""The call families whose single and batched entry points share one driver, and the one driver of every MSM over raw bases, under the
functional HIP emulation: (1) GA_MSM_MAX_CHUNK reaches the prover's MSMs over plain vectors, a window share and ga_g16_commit, and the
proof does not change; (2) a single call is the batched call with count = 1, byte for byte, from host pointers and from device
buffers; (3) a refusal names the entry point that was called, the Groth16 entry points included (g16_abi.hip); (4) ga_g16_h_chain_dev is
ga_g16_h_chain without the upload (one driver).  The correctness anchors of the singles (pyref, the C oracle) stay in
test_emu_kernels.py / test_gpu_parity.py; tests/test_abi_drivers_gpu.py runs these cases on the device at its sizes."""
import ctypes as C

import numpy as np
import pytest

import oracle
import test_plonk_batch as pb
import test_prove_batch as gb
from gnark_amd import _lib, ecc, fft, groth16
from gnark_amd.device import jac_words
from helpers import BLS12_381, BN254, arr_to_g1_affine, jac_to_affine_py

CURVES = [BN254, BLS12_381]
GA_ERR_INVALID = -1
KNOB = "GA_MSM_MAX_CHUNK"
_ptr = lambda a: a.ctypes.data_as(C.c_void_p)


# ---- 1. the chunk loop of msm_run under the prover -------------------------------------------------------------------------------
def _proofs(ctx, c, logn):
    """(the proof under the plain key, the proof summed from the two window shares of it): every MSM is over un-pinned vectors"""
    sol, r, s = gb.solutions(ctx, c, logn, 1)[0]
    pk = gb.pin(ctx, c, logn, "plain")
    try:
        gb.check_layout(pk, "plain")
        whole = groth16.Prove(pk, sol, gb.NB_PUBLIC, r, s)
    finally:
        pk.FreeGPUResources()
    shares = [gb.pin(ctx, c, logn, "plain", window_shard=(i, 2)) for i in range(2)]
    try:
        assert [groth16.ShardLayout(p)["win_index"] for p in shares] == [0, 1]
        parts = [groth16.ProvePartial(p, sol, gb.NB_PUBLIC) for p in shares]
        summed = groth16.Finish(shares[0], groth16.SumPartials(c.name, parts, lib=ctx.lib), r, s)
    finally:
        for p in shares:
            p.FreeGPUResources()
    return whole, summed


def case_prover_chunks(ctx, monkeypatch, c, logn, chunk):
    """`chunk` cuts every base vector of the key (2^logn - 1 .. 2^logn - 3 points) into at least three chunks with a ragged last one:
    the proof bytes are those with the knob unset, whole and summed from window shares 0 and 1 of 2 (share 1: win_lo > 0 in the chunk
    loop), and the points are the C oracle's"""
    n = 1 << logn
    assert all(2 * chunk < m and m % chunk for m in (n - 1, n - 2, n - 3))   # Z; B, G2.B; A, K
    want = gb.oracle_proofs(ctx, c, logn, "plain", 1)
    monkeypatch.delenv(KNOB, raising=False)
    plain = _proofs(ctx, c, logn)
    monkeypatch.setenv(KNOB, str(chunk))
    try:
        chunked = _proofs(ctx, c, logn)
    finally:
        monkeypatch.delenv(KNOB)
    for what, a, b in zip(("whole", "window shares"), plain, chunked):
        assert a.WriteTo() == b.WriteTo(), what
        gb.assert_proofs([b], want, what)


def case_commit_chunks(ctx, monkeypatch, c, logn, chunk):
    """ga_g16_commit over a commitment key of 2^logn - 7 points: commitment and proof of knowledge (affine images) are the same bytes
    with and without the knob, and the C oracle's MSMs over the two bases"""
    m = (1 << logn) - 7
    assert 2 * chunk < m and m % chunk
    basis, sigma = gb._gen(ctx, c, 0, m, 8), gb._gen(ctx, c, 0, m, 9)
    values = gb._scal(ctx, c, m, 77)
    pk = gb.pin(ctx, c, logn, "plain", commitment_keys=[(basis, sigma)])
    try:
        monkeypatch.delenv(KNOB, raising=False)
        plain = pk.Commit(0, values)
        monkeypatch.setenv(KNOB, str(chunk))
        try:
            chunked = pk.Commit(0, values)
        finally:
            monkeypatch.delenv(KNOB)
    finally:
        pk.FreeGPUResources()
    for what, bases, a, b in zip(("commitment", "pok"), (basis, sigma), plain, chunked):
        assert np.array_equal(a, b), what
        assert arr_to_g1_affine(c, b) == jac_to_affine_py(c, 0, oracle.msm(c.cid, 0, bases, values, nthreads=4)), what


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_prover_chunks(emu_ctx, monkeypatch, c):
    """2^6 constraints under the emulation (2^10 on the device), 20 points per chunk: 20 + 20 + 20 + a ragged rest"""
    case_prover_chunks(emu_ctx, monkeypatch, c, 6, 20)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_commit_chunks(emu_ctx, monkeypatch, c):
    case_commit_chunks(emu_ctx, monkeypatch, c, 6, 18)


# ---- 2. single is count = 1 ------------------------------------------------------------------------------------------------------
def _on_device(ctx, arrays, call, out_shape, out_index=None):
    """call(pointers of device copies of `arrays`[, pointer of an output buffer]) -> the output buffer (or copy out_index) on the host"""
    bufs = [ctx.to_device(a) for a in arrays]
    out = ctx.malloc(int(np.prod(out_shape)) * 8) if out_index is None else bufs[out_index]
    try:
        call(*([b.ptr for b in bufs] + ([out.ptr] if out_index is None else [])))
        return out.to_host(out_shape)
    finally:
        for b in bufs + ([out] if out_index is None else []):
            b.free()


def case_fft_single_is_batch(ctx, c, logn, count=3):
    lib, n = ctx.lib, 1 << logn
    vecs, _ = gb._vectors(c, logn, count)
    d = fft.Domain(ctx, c.name, n)
    try:
        for inv, dec, coset in gb.FFT_MODES:
            batch = gb._run(d, inv)(np.stack(vecs), dec, coset)
            dbatch = _on_device(ctx, [np.stack(vecs)], lambda p: lib.check(lib.ga_fft_batch(d.handle, p, count, int(inv), dec, int(coset), 1)), (count, n, 4), 0)
            assert np.array_equal(batch, dbatch)
            for j in range(count):
                single = (d.FFTInverse if inv else d.FFT)(vecs[j], dec, coset)
                dsingle = _on_device(ctx, [vecs[j]], lambda p: lib.check(lib.ga_fft(d.handle, p, int(inv), dec, int(coset), 1)), (n, 4), 0)
                assert np.array_equal(single, batch[j]) and np.array_equal(dsingle, batch[j]), (inv, dec, coset, j)
            one = gb._run(d, inv)(vecs[0][None], dec, coset)
            assert np.array_equal(one[0], batch[0])
    finally:
        d.close()


def case_compute_h_single_is_batch(ctx, c, logn, short, count=3):
    lib, n = ctx.lib, 1 << logn
    T = gb._h_triples(c, logn, short, count)
    A, B, Cc = (np.stack([t[k] for t in T]) for k in range(3))
    d = fft.Domain(ctx, c.name, n)
    try:
        batch = d.compute_h_batch(A, B, Cc)
        dbatch = _on_device(ctx, [A, B, Cc], lambda a, b, cc, o: lib.check(lib.ga_compute_h_batch(d.handle, a, b, cc, count, n - short, o, 1)), (count, n, 4))
        assert np.array_equal(batch, dbatch)
        for j in range(count):
            single = d.compute_h(A[j], B[j], Cc[j])
            dsingle = _on_device(ctx, [A[j], B[j], Cc[j]], lambda a, b, cc, o: lib.check(lib.ga_compute_h(d.handle, a, b, cc, n - short, o, 1)), (n, 4))
            assert np.array_equal(single, batch[j]) and np.array_equal(dsingle, batch[j]), j
        assert np.array_equal(d.compute_h_batch(A[:1], B[:1], Cc[:1])[0], batch[0])
    finally:
        d.close()


def case_kzg_single_is_batch(ctx, c, length, count=3):
    """an SRS of length + 5 points: the claimed value and the Jacobian image of H of the single call are the bytes of row 0 of a batch
    of one and of row j of a batch of three (row j of a batched table MSM depends on vector j alone)"""
    lib, jw = ctx.lib, jac_words(c.cid, 0)
    polys, points = pb.open_inputs(c, length, count)
    table = ecc.PrecomputedBases(ctx, c.name, 0, pb.srs_of(c, length + 5)[1])

    def batch(rows, flags, ptrs):
        vals, H = np.zeros((len(rows), 4), np.uint64), np.zeros((len(rows), jw), np.uint64)
        arr = (C.c_void_p * len(rows))(*ptrs)
        lib.check(lib.ga_kzg_open_batch(table.handle, arr, length, len(rows), flags, _ptr(np.ascontiguousarray(points[rows])), _ptr(vals), _ptr(H)))
        return vals, H

    def single(j, flags, ptr):
        val, H = np.zeros(4, np.uint64), np.zeros(jw, np.uint64)
        lib.check(lib.ga_kzg_open(table.handle, ptr, length, flags, _ptr(np.ascontiguousarray(points[j])), _ptr(val), _ptr(H)))
        return val, H
    bufs = [ctx.to_device(polys[j]) for j in range(count)]
    try:
        rows = list(range(count))
        for flags, ptrs in ((0, [polys[j].ctypes.data for j in rows]), (_lib.SCALARS_ON_DEVICE, [b.ptr for b in bufs])):
            v3, H3 = batch(rows, flags, ptrs)
            for j in rows:
                sv, sH = single(j, flags, C.c_void_p(ptrs[j]))
                v1, H1 = batch([j], flags, ptrs[j:j + 1])
                assert np.array_equal(sv, v1[0]) and np.array_equal(sH, H1[0]), (flags, j, "count = 1")
                assert np.array_equal(sv, v3[j]) and np.array_equal(sH, H3[j]), (flags, j, "count = 3")
    finally:
        for b in bufs:
            b.free()
        table.free()


def case_table_run_shapes(ctx, c, group, n):
    """ga_msm_table_run, ga_msm_table_run_windows over [0, nwin) and ga_msm_table_run_batch with k = 1: one Jacobian image"""
    lib = ctx.lib
    P = gb._gen(ctx, c, group, n, 21 + group)
    S = gb._scal(ctx, c, n, 23)
    table = ecc.PrecomputedBases(ctx, c.name, group, P)
    buf = ctx.to_device(S)
    try:
        nwin = table.info()["windows"]
        for scal in (S, buf):
            run = table.MultiExp(scal)
            assert np.array_equal(run, table.MultiExpWindows(scal, 0, nwin))
            assert np.array_equal(run, table.MultiExpBatch([scal])[0])
        assert np.array_equal(table.MultiExp(S), table.MultiExp(buf))
        assert jac_to_affine_py(c, group, run) == jac_to_affine_py(c, group, oracle.msm(c.cid, group, P, S, nthreads=4))
    finally:
        buf.free()
        table.free()


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_fft_single_is_batch(emu_ctx, c):
    case_fft_single_is_batch(emu_ctx, c, 6)


@pytest.mark.parametrize("short", [5, 0], ids=["n-5", "n"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_compute_h_single_is_batch(emu_ctx, c, short):
    case_compute_h_single_is_batch(emu_ctx, c, 6, short)


@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_kzg_single_is_batch(emu_ctx, monkeypatch, c):
    monkeypatch.delenv("GA_PLONK_BATCH_MAX", raising=False)
    case_kzg_single_is_batch(emu_ctx, c, 1 << 6)


@pytest.mark.parametrize("c,group", [(BN254, 0), (BN254, 1), (BLS12_381, 0)], ids=["bn254-g1", "bn254-g2", "bls12-381-g1"])
def test_table_run_shapes(emu_ctx, c, group):
    case_table_run_shapes(emu_ctx, c, group, 1 << 6)


# ---- 3. a refusal names the entry point that was called --------------------------------------------------------------------------
def case_refusal_names(ctx, c=BN254, n=8):
    """one null or out-of-range argument that an entry point shares with its twin: GA_ERR_INVALID under its own name"""
    lib = ctx.lib
    v = np.zeros((n, 4), np.uint64)
    out = np.zeros((n, 4), np.uint64)
    jac = np.zeros(jac_words(c.cid, 0), np.uint64)
    one = (C.c_void_p * 1)(v.ctypes.data)
    null1 = (C.c_void_p * 1)(None)
    d = fft.Domain(ctx, c.name, n)
    table = ecc.PrecomputedBases(ctx, c.name, 0, pb.srs_of(c, n)[1])
    short = ecc.PrecomputedBases(ctx, c.name, 0, pb.srs_of(c, n)[1][:2])
    P = _ptr
    calls = {
        "ga_fft": lambda: lib.ga_fft(d.handle, None, 0, 0, 0, 0),
        "ga_fft_batch": lambda: lib.ga_fft_batch(d.handle, None, 2, 0, 0, 0, 0),
        "ga_compute_h": lambda: lib.ga_compute_h(d.handle, P(v), P(v), P(v), n + 1, P(out), 0),
        "ga_compute_h_batch": lambda: lib.ga_compute_h_batch(d.handle, P(v), P(v), P(v), 1, n + 1, P(out), 0),
        "ga_kzg_open": lambda: lib.ga_kzg_open(short.handle, P(v), n, 0, P(v), P(out), P(jac)),
        "ga_kzg_open_batch": lambda: lib.ga_kzg_open_batch(short.handle, one, n, 1, 0, P(v), P(out), P(jac)),
        "ga_msm_table_run": lambda: lib.ga_msm_table_run(table.handle, None, 0, P(jac)),
        "ga_msm_table_run_windows": lambda: lib.ga_msm_table_run_windows(table.handle, None, 0, 0, 1, P(jac)),
        "ga_msm_table_run_batch": lambda: lib.ga_msm_table_run_batch(table.handle, null1, 1, 0, P(jac)),
        "ga_msm": lambda: lib.ga_msm(ctx.handle, c.cid, 0, None, P(v), n, 0, P(jac)),
        "ga_msm_windows": lambda: lib.ga_msm_windows(ctx.handle, c.cid, 0, None, P(v), n, 0, 0, 1, P(jac), None, None),
        "ga_gen_bases": lambda: lib.ga_gen_bases(ctx.handle, 99, 0, 1, n, None, None),
        "ga_gen_bases_at": lambda: lib.ga_gen_bases_at(ctx.handle, 99, 0, 1, 0, n, None, None),
        "ga_fr_vec_mul": lambda: lib.ga_fr_vec_mul(ctx.handle, c.cid, None, P(v), n, P(out), 0),
        "ga_fr_poly_evaluate": lambda: lib.ga_fr_poly_evaluate(ctx.handle, c.cid, None, n, P(v), P(out), 0),
    }
    try:
        for name, call in calls.items():
            assert call() == GA_ERR_INVALID, name
            msg = lib.ga_last_error().decode()
            assert msg.startswith(name + ":") or msg.startswith(name + " "), (name, msg)
        # the valid calls still work afterwards
        assert np.array_equal(d.FFTInverse(d.FFT(v, fft.DIF), fft.DIT), v)
        table.MultiExp(v)
    finally:
        short.free()
        table.free()
        d.close()


def test_refusal_names(emu_ctx):
    case_refusal_names(emu_ctx)


def case_g16_refusal_names(ctx, c=BN254, logn=3):
    """the Groth16 half: one refusing call per Groth16 entry point that takes a pointer or a handle -- the argument null, or n = 0
    keys for ga_g16_prove_multi -- gives GA_ERR_INVALID under the name that was called, and the key then proves the bytes it proved
    before.  One tiny key: nothing here depends on size."""
    from gnark_amd import synth
    lib, cid, h = ctx.lib, c.cid, ctx.handle
    inst = synth.make_instance(ctx, c.name, logn, 0x6A16, want_dlogs=False)
    pk = inst.proving_key(ctx, precompute=1)
    k = pk.handle
    out, n32, sz = C.c_void_p(), C.c_uint32(), C.c_size_t()
    v = np.zeros((1 << logn, 4), np.uint64)
    keys0 = (C.c_void_p * 1)(k)
    N = None
    calls = {
        "ga_g16_pk_create": lambda: lib.ga_g16_pk_create(h, N, C.byref(out)),
        "ga_g16_builder_create": lambda: lib.ga_g16_builder_create(N, cid, 1 << logn, 1 << logn, 0, 1, C.byref(out)),
        "ga_g16_builder_reserve": lambda: lib.ga_g16_builder_reserve(N, 0, 1),
        "ga_g16_builder_append": lambda: lib.ga_g16_builder_append(N, 0, _ptr(v), 1),
        "ga_g16_builder_set_point": lambda: lib.ga_g16_builder_set_point(N, 0, _ptr(v)),
        "ga_g16_builder_set_infinity": lambda: lib.ga_g16_builder_set_infinity(N, 0, _ptr(v), 1),
        "ga_g16_builder_add_commitment_key": lambda: lib.ga_g16_builder_add_commitment_key(N, _ptr(v), _ptr(v), 1),
        "ga_g16_builder_set_k_remove": lambda: lib.ga_g16_builder_set_k_remove(N, _ptr(v), 1),
        "ga_g16_builder_set_window_shard": lambda: lib.ga_g16_builder_set_window_shard(N, 0, 1),
        "ga_g16_builder_finish": lambda: lib.ga_g16_builder_finish(N, 0, C.byref(out)),
        "ga_g16_shard_layout": lambda: lib.ga_g16_shard_layout(k, N),
        "ga_g16_table_layout": lambda: lib.ga_g16_table_layout(k, N),
        "ga_g16_pk_read_mem": lambda: lib.ga_g16_pk_read_mem(h, cid, N, 0, 0, 0, 1, N, 0, C.byref(out), N),
        "ga_g16_pk_read_fd": lambda: lib.ga_g16_pk_read_fd(h, cid, -1, 0, 0, 1, N, 0, C.byref(out), N),
        "ga_g16_pk_read_mem_checked": lambda: lib.ga_g16_pk_read_mem_checked(h, cid, N, 0, 0, 0, 1, N, 0, C.byref(out), N),
        "ga_g16_pk_read_fd_checked": lambda: lib.ga_g16_pk_read_fd_checked(h, cid, -1, 0, 0, 1, N, 0, C.byref(out), N),
        "ga_g16_key_write_fd": lambda: lib.ga_g16_key_write_fd(h, N, 0, 1, N),
        "ga_g16_proof_unmarshal": lambda: lib.ga_g16_proof_unmarshal(cid, N, 0, _ptr(v), N, 0, C.byref(n32), N, C.byref(sz)),
        "ga_point_unmarshal": lambda: lib.ga_point_unmarshal(cid, 0, N, 0, _ptr(v), C.byref(sz)),
        "ga_g16_proof_marshal": lambda: lib.ga_g16_proof_marshal(cid, N, _ptr(v), v.nbytes, C.byref(sz)),
        "ga_g16_proof_marshal_bsb22": lambda: lib.ga_g16_proof_marshal_bsb22(cid, N, N, 0, N, _ptr(v), v.nbytes, C.byref(sz)),
        "ga_g16_proof_marshal_raw": lambda: lib.ga_g16_proof_marshal_raw(cid, N, N, 0, N, _ptr(v), v.nbytes, C.byref(sz)),
        "ga_g1_marshal_uncompressed": lambda: lib.ga_g1_marshal_uncompressed(cid, N, _ptr(v), v.nbytes, C.byref(sz)),
        "ga_g16_prove": lambda: lib.ga_g16_prove(k, N, _ptr(v), _ptr(v), _ptr(v), 1, inst.nb_public, _ptr(v), _ptr(v), _ptr(v)),
        "ga_g16_prove_batch": lambda: lib.ga_g16_prove_batch(k, 1, N, N, N, N, 1, inst.nb_public, _ptr(v), _ptr(v), _ptr(v)),
        "ga_g16_prove_oneshot": lambda: lib.ga_g16_prove_oneshot(h, N, _ptr(v), _ptr(v), _ptr(v), _ptr(v), 1, inst.nb_public, _ptr(v), _ptr(v), _ptr(v)),
        "ga_g16_prove_partial": lambda: lib.ga_g16_prove_partial(k, N, _ptr(v), _ptr(v), _ptr(v), 1, inst.nb_public, _ptr(v)),
        "ga_g16_finish": lambda: lib.ga_g16_finish(k, N, _ptr(v), _ptr(v), _ptr(v)),
        "ga_g16_witness_partial": lambda: lib.ga_g16_witness_partial(k, N, inst.nb_public, _ptr(v)),
        "ga_g16_h_chain": lambda: lib.ga_g16_h_chain(k, _ptr(v), 1, N),
        "ga_g16_h_chain_dev": lambda: lib.ga_g16_h_chain_dev(k, N, 1),
        "ga_g16_h_combine": lambda: lib.ga_g16_h_combine(k, N, N, N),
        "ga_g16_z_partial": lambda: lib.ga_g16_z_partial(k, N, _ptr(v)),
        "ga_g16_prove_multi": lambda: lib.ga_g16_prove_multi(keys0, 0, _ptr(v), _ptr(v), _ptr(v), _ptr(v), 1, inst.nb_public, _ptr(v), _ptr(v), _ptr(v)),
        "ga_g16_commit": lambda: lib.ga_g16_commit(k, 0, N, 1, _ptr(v), _ptr(v)),
        "ga_g16_fold_pok": lambda: lib.ga_g16_fold_pok(cid, _ptr(v), 1, N, _ptr(v)),
        "ga_g16_lane_stats": lambda: lib.ga_g16_lane_stats(h, N),
    }
    try:
        args = (pk, inst.solution, inst.nb_public, inst.r, inst.s)
        before = groth16.Prove(*args).WriteTo()
        for name, call in calls.items():
            assert call() == GA_ERR_INVALID, (name, lib.ga_last_error().decode())
            msg = lib.ga_last_error().decode()
            assert msg.startswith(name + ":") or msg.startswith(name + " "), (name, msg)
        assert out.value is None
        assert groth16.Prove(*args).WriteTo() == before
    finally:
        pk.FreeGPUResources()


def test_g16_refusal_names(emu_ctx):
    case_g16_refusal_names(emu_ctx)


# ---- 4. ga_g16_h_chain_dev is ga_g16_h_chain without the upload ------------------------------------------------------------------
def case_h_chain_dev_is_h_chain(ctx, c, logn, short):
    """v of n - short elements: the chain of the host vector (upload, pad, transform) and the chain of a device buffer that holds v
    already (pad, transform) leave the same n * 32 bytes.  Both buffers start with stale non-zero bytes everywhere, so the tails are
    what the pads wrote; n_constraints = n + 1 is refused."""
    from gnark_amd import synth
    n = 1 << logn
    m = n - short
    pk = synth.make_instance(ctx, c.name, logn, 0x6C4A, want_dlogs=False).proving_key(ctx, precompute=1)
    v = gb._scal(ctx, c, m, 0x6C4B)
    stale = np.full((n, 4), 0x0123456789ABCDEF, np.uint64)
    filled = stale.copy()
    filled[:m] = v
    buf_a, buf_b = ctx.to_device(stale), ctx.to_device(filled)
    try:
        groth16.HChain(pk, v, buf_a.ptr)
        groth16.HChainDevice(pk, buf_b.ptr, m)
        a, b = buf_a.to_host((n, 4)), buf_b.to_host((n, 4))
        assert np.array_equal(a, b)
        assert not np.array_equal(a, stale)
        assert ctx.lib.ga_g16_h_chain_dev(pk.handle, buf_b.ptr, n + 1) == GA_ERR_INVALID
        assert "exceed the domain cardinality" in ctx.lib.ga_last_error().decode()
        assert np.array_equal(buf_b.to_host((n, 4)), b)   # (refused before anything was written)
    finally:
        buf_a.free()
        buf_b.free()
        pk.FreeGPUResources()


@pytest.mark.parametrize("short", [0, 3], ids=["n", "n-3"])
@pytest.mark.parametrize("c", CURVES, ids=lambda c: c.name)
def test_h_chain_dev_is_h_chain(emu_ctx, c, short):
    case_h_chain_dev_is_h_chain(emu_ctx, c, 3, short)

#!/usr/bin/env python3
"""Times ga_plonk_verify (gnark_amd/csrc/plonk_verify.hip.h) on the device and writes profiles/plonk_verify.json.

    python tools/plonk_verify_bench.py [--log-count 12 16] [--public 1 64] [--reps 10] [--g16-reps 3] [--curves bn254 bls12-381]

One process.  Per curve, number of public inputs and count: `count` proofs tiled from four valid ones of the Python prover of
tests/plonk_verify_cases.py (one BSB22 commitment; a domain of 16 rows for one public input, 128 for 64), every operand on the device,
the C call itself (no Python packing inside the timed region).  Reported: the median of `reps` wall-clock calls and proofs per second
for the default mode (one verdict per proof) and for GA_PLONK_VERIFY_COMBINED, and one profiled call's stage times: the new kernels
(plonk_vf_public, plonk_vf_rows, plonk_vf_combine) beside the point check, the sparse sum or the MSM, and the pairing.  The sum of the
stages is device time; the rest of the wall clock is host work -- in the default mode above all the sparse sum's classification of
count * (2 (9 + nb_bsb) + 2) coefficients on the host.

Interleaved in the same process, as the only yardstick the project has: g16_verify.VerifyMany / BatchVerify on the same counts, one
public input, Python packing included (that is how they are called).  There is no CPU figure: gnark-crypto is not available to this
repository, and none is made up."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

NEW_STAGES = ("plonk_vf_public", "plonk_vf_rows", "plonk_vf_combine")


def stage_groups(st):
    """the profiler's stages by the call they belong to"""
    g = {k: round(st.get(k, 0.0), 3) for k in NEW_STAGES}
    fam = {"check_points": ("check_",), "sparse_sum": ("sparse_", "scale_"), "msm": ("msm", "sort", "bucket", "reduce", "digits", "tasks", "window"),
           "pairing": ("pairing_",)}
    rest = 0.0
    for k, v in st.items():
        if k in NEW_STAGES:
            continue
        for name, prefixes in fam.items():
            if k.startswith(prefixes):
                g[name] = round(g.get(name, 0.0) + v, 3)
                break
        else:
            rest += v
    g["other"] = round(rest, 3)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-count", type=int, nargs="+", default=[12, 16])
    ap.add_argument("--public", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--g16-reps", type=int, default=3)
    ap.add_argument("--curves", nargs="+", default=["bn254", "bls12-381"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_verify.json"))
    args = ap.parse_args()

    import gnark_amd
    import plonk_verify_cases as pc
    import pyref
    from gnark_amd import _lib, ecc, g16_verify, groth16
    from gnark_amd import plonk_verify as pv
    from gnark_amd.device import affine_words, curve_id
    from helpers import fr_to_arr, gen_of, pts_to_arr

    results, yardstick = [], []
    with gnark_amd.Context(0) as ctx:
        lib = ctx.lib

        def profiled(call):
            ctx.profile(True)
            ctx.profile_reset()
            call()
            st = {}
            for name, ms in ctx.profile_read():
                st[name] = st.get(name, 0.0) + ms
            ctx.profile(False)
            return st

        def g16_run(curve, N):
            """pairing_bench's proofs from known logarithms: VerifyMany and BatchVerify wall clock, one public input"""
            cid = curve_id(curve)
            c = pyref.CURVES[curve]
            w1, w2, r = affine_words(cid, 0), affine_words(cid, 1), c.r
            rng = np.random.default_rng(0x16 + cid)

            def rand_ints(m):
                w = rng.integers(0, 1 << 64, size=(m, 4), dtype=np.uint64)
                w[:, 3] = rng.integers(1, r >> 192, size=m, dtype=np.uint64)
                return [int.from_bytes(row.tobytes(), "little") for row in w]

            def mul(group, ks, m):
                words = np.array([[(k >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for k in ks], dtype=np.uint64)
                buf = ecc.BatchScalarMultiplication(ctx, curve, group, pts_to_arr(c, group, [gen_of(c, group)]), words, out_device=True)
                try:
                    return buf.to_host((m, w1 if group == 0 else w2))
                finally:
                    buf.free()
            a, b, g, d, k0, k1 = rand_ints(6)
            hdr1, hdr2 = mul(0, [a, k0, k1], 3), mul(1, [b, g, d], 3)
            vk = g16_verify.VerifyingKey(cid, hdr1[0], hdr2[0], hdr2[1], hdr2[2], hdr1[1:3].copy())
            xs, ys, pws = rand_ints(N), rand_ints(N), rand_ints(N)
            dinv = pow(d, -1, r)
            zs = [(x * y - a * b - (k0 + pw * k1) * g) * dinv % r for x, y, pw in zip(xs, ys, pws)]
            Ar, Bs, Krs = mul(0, xs, N), mul(1, ys, N), mul(0, zs, N)
            proofs = [groth16.Proof(cid, Ar[i], Bs[i], Krs[i], lib) for i in range(N)]
            witnesses = [[pw] for pw in pws]
            return {"VerifyMany": lambda: bool(g16_verify.VerifyMany(ctx, vk, proofs, witnesses).all()),
                    "BatchVerify": lambda: g16_verify.BatchVerify(ctx, vk, proofs, witnesses, np.random.default_rng(1))}

        for curve in args.curves:
            c = pyref.CURVES[curve]
            cid = curve_id(curve)
            for nb_public in args.public:
                n = 16
                while n < nb_public + 1:
                    n *= 2
                cir = pc.circuit(curve, n, 1, nb_public)
                distinct = [cir.prove(seed) for seed in range(4)]
                for p, ch in distinct:
                    assert pc.model_verify(c, cir.key, p, cir.pub, ch) == (True, True)
                vk = cir.key.device(ctx)
                np_pts, W = 9 + vk.nb_bsb, 2 * (9 + vk.nb_bsb) + 2
                packed = pv._pack(vk, [pc.to_proof(c, p) for p, _ in distinct], [cir.pub] * 4, pc.chal_arr(c, [ch for _, ch in distinct]),
                                  [fr_to_arr(c, cir.hashes)] * 4, lib)[:5]
                for logc in args.log_count:
                    N = 1 << logc
                    tiled = [np.ascontiguousarray(np.concatenate([np.asarray(a).reshape(4, -1)] * (N // 4))) for a in packed]
                    bufs = [ctx.to_device(a) for a in tiled]
                    d_ok, d_rel = ctx.malloc(N), ctx.malloc(N)
                    a = _lib.PlonkProofs()
                    a.points, a.evals, a.challenges, a.public_inputs, a.bsb_hashes = (b.ptr for b in bufs)
                    out2 = (C.c_uint64 * 2)()
                    words = np.random.default_rng(7).integers(0, 1 << 64, size=(N, 2), dtype=np.uint64)
                    weights = pv.fr_mont(cid, [int(lo) | (int(hi) << 64) for lo, hi in words])
                    g16 = g16_run(curve, N) if nb_public == args.public[0] else {}

                    def run(flags):
                        lib.check(lib.ga_plonk_verify(vk.handle, C.byref(a), N, _lib.PLONK_ON_DEVICE | flags, weights.ctypes.data_as(C.c_void_p),
                                                      C.c_void_p(d_ok.ptr), C.c_void_p(d_rel.ptr), out2))
                        assert (out2[0], out2[1]) == (0, 0xFFFFFFFFFFFFFFFF), tuple(out2)

                    modes = {"default": 0, "combined": _lib.PLONK_VERIFY_COMBINED}
                    secs = {k: [] for k in list(modes) + list(g16)}
                    for rep in range(args.reps + 1):                        # rep 0 warms up: the scratch exists afterwards
                        for name, flags in modes.items():
                            t0 = time.perf_counter()
                            run(flags)
                            if rep:
                                secs[name].append(time.perf_counter() - t0)
                        if rep <= args.g16_reps:
                            for name, call in g16.items():                  # interleaved with the PLONK calls
                                t0 = time.perf_counter()
                                assert call() is True, name
                                ctx.sync()
                                if rep:
                                    secs[name].append(time.perf_counter() - t0)
                    rec = {"curve": curve, "count": N, "nb_public": nb_public, "nb_bsb": 1, "domain": n, "reps": args.reps}
                    for name, flags in modes.items():
                        med = statistics.median(secs[name])
                        st = profiled(lambda: run(flags))
                        groups = stage_groups(st)
                        device_ms = round(sum(st.values()), 3)
                        rec[name] = {"median_s": round(med, 5), "proofs_per_s": round(N / med), "stage_ms": groups, "device_ms": device_ms,
                                     "new_kernels_share_of_device_time": round(sum(groups[k] for k in NEW_STAGES) / device_ms, 4) if device_ms else None}
                    assert ctx and d_ok.to_host((N,), dtype=np.uint8).all()
                    results.append(rec)
                    print("PLONK_VERIFY_RESULT " + json.dumps(rec), flush=True)
                    if g16:
                        y = {"curve": curve, "count": N, "public_inputs": 1, "reps": min(args.reps, args.g16_reps)}
                        for name in g16:
                            med = statistics.median(secs[name])
                            y[name] = {"median_s": round(med, 4), "proofs_per_s": round(N / med)}
                        yardstick.append(y)
                        print("G16_VERIFY_YARDSTICK " + json.dumps(y), flush=True)
                    for b in bufs + [d_ok, d_rel]:
                        b.free()
                vk.close()
    doc = {"device_results": results, "groth16_yardstick": yardstick,
           "note": "wall clock of the C call with every operand on the device (median); stage_ms is one profiled call, grouped by the call a stage "
                   "belongs to; the groth16 figures are g16_verify.VerifyMany / BatchVerify in the same process with their Python packing, as they are "
                   "called.  Measured on one MI355X box.",
           "cpu_reference": None, "cpu_reference_note": "gnark-crypto was not available where this was measured: no CPU figure"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

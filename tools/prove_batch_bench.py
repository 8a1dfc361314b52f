#!/usr/bin/env python3
"""Times ga_g16_prove_batch (many witnesses under one key in one device pass, gnark_amd/csrc/groth16.hip) against a sequential loop
of ga_g16_prove on a library built from the PARENT commit, and writes profiles/prove_batch.json.

    tools/build_variant.sh is for compile-time knobs; the baseline here is another checkout:
        git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/gnark_amd/csrc -j8 TARGET=$PWD/gnark_amd/variants/libgnark_amd_parent.so
    python tools/prove_batch_bench.py [--parent-lib gnark_amd/variants/libgnark_amd_parent.so] [--log-n 10 12 14 16] [--counts 4 16 64]
                                      [--reps 10] [--out profiles/prove_batch.json]

Every configuration (curve, size) runs in a child process of its own under `timeout`; the first child that fails ends the run.  Both
libraries are loaded into that one process, each with its own context and its own copy of the key pinned with all tables
(precompute = 1), and the timed runs are interleaved: batch, sequential loop, batch, ...  A timed region starts and ends with ga_sync
on its context; the figure is the median wall-clock time of `reps` repetitions after one warm-up of each side.  Per configuration the
file records
  * wall-clock per proof of ga_g16_prove_batch and of the parent build's loop of ga_g16_prove over the same solutions (the baseline:
    the new build's own single-proof path is not), and whether the proof bytes agree;
  * the stage breakdown of one batch from the stage profiler (hipEvents around every launch), taken in a separate pass;
  * ga_compute_h_batch at count 16 against 16 x ga_compute_h of the parent build (2^10 and 2^14), host pointers on both sides;
  * one sanity line: ga_g16_prove (single) of the new build against the parent build (2^10 and 2^20)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CURVES = ("bn254", "bls12-381")
TAG = "PROVE_BATCH_RESULT "


def timed(ctx, call):
    ctx.sync()
    t0 = time.perf_counter()
    call()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3


def interleaved(reps, sides):
    """sides: [(ctx, call)]; one warm-up each, then reps rounds of every side in turn; the medians in ms"""
    for ctx, call in sides:
        timed(ctx, call)
    ms = [[] for _ in sides]
    for _ in range(reps):
        for k, (ctx, call) in enumerate(sides):
            ms[k].append(timed(ctx, call))
    return [statistics.median(v) for v in ms], [min(v) for v in ms]


def older_library(path):
    """a build of an earlier commit through the current prototypes: entry points it does not have yet stay unbound"""
    import ctypes
    from gnark_amd import _lib
    lib = _lib.Library.__new__(_lib.Library)
    lib.path, lib.dll = path, ctypes.CDLL(path)
    for name, (res, args) in _lib._PROTOS.items():
        try:
            fn = getattr(lib.dll, name)
        except AttributeError:
            continue
        fn.restype, fn.argtypes = res, args
        setattr(lib, name, fn)
    return lib


def contexts(parent_lib):
    import gnark_amd
    new = gnark_amd.Context(0)
    par = gnark_amd.Context(0, lib=older_library(parent_lib))
    return new, par


def solutions_of(ctx, inst, count):
    """`count` distinct solutions of the instance's shape (uniform W with W[0] = 1, A, B, C = A o B) with their own (r, s)"""
    import numpy as np
    from gnark_amd import groth16, synth
    cid, m = inst.curve, inst.solution.A.shape[0]
    out = []
    for j in range(count):
        seed = 0xBA7C4 + 16 * j
        W = synth._gen_scalars(ctx, cid, inst.nb_wires, seed)
        W[0] = inst.solution.W[0]
        a, b = synth._gen_scalars(ctx, cid, m, seed + 1), synth._gen_scalars(ctx, cid, m, seed + 2)
        c = np.zeros_like(a)
        ctx.lib.check(ctx.lib.ga_fr_vec_mul(ctx.handle, cid, a.ctypes.data, b.ctypes.data, m, c.ctypes.data, 0))
        rs = synth._gen_scalars(ctx, cid, 2, seed + 3)
        out.append((groth16.Solution(W, a, b, c), rs[0].copy(), rs[1].copy()))
    return out


def stage_profile(ctx, call):
    ctx.profile(True)
    ctx.profile_reset()
    call()
    st = {}
    for name, ms in ctx.profile_read():
        st[name] = st.get(name, 0.0) + ms
    ctx.profile_reset()
    ctx.profile(False)
    return {k: round(v, 4) for k, v in sorted(st.items(), key=lambda kv: -kv[1])}


def run_prove(curve, logn, counts, reps, parent_lib):
    import numpy as np
    from gnark_amd import groth16, synth
    new, par = contexts(parent_lib)
    inst = synth.make_instance(new, curve, logn, want_dlogs=False)
    sols = solutions_of(new, inst, max(counts))
    pk_new, pk_par = inst.proving_key(new, precompute=1), inst.proving_key(par, precompute=1)
    lay = groth16.ShardLayout(pk_new)
    rows = []
    try:
        for count in counts:
            S = sols[:count]
            rs, ss = np.stack([x[1] for x in S]), np.stack([x[2] for x in S])
            batch = lambda: groth16.ProveBatch(pk_new, [x[0] for x in S], inst.nb_public, rs, ss)
            loop = lambda: [groth16.Prove(pk_par, x[0], inst.nb_public, x[1], x[2]) for x in S]
            same = [p.raw().tobytes() for p in batch()] == [p.raw().tobytes() for p in loop()]
            (b_ms, l_ms), (b_min, l_min) = interleaved(reps, [(new, batch), (par, loop)])
            rows.append({"count": count, "batch_ms_per_proof": round(b_ms / count, 4), "parent_sequential_ms_per_proof": round(l_ms / count, 4),
                         "speedup": round(l_ms / b_ms, 3), "batch_min_ms_per_proof": round(b_min / count, 4),
                         "parent_sequential_min_ms_per_proof": round(l_min / count, 4), "proof_bytes_equal": same,
                         "batch_stages_ms": stage_profile(new, batch)})
    finally:
        pk_new.FreeGPUResources()
        pk_par.FreeGPUResources()
    res = {"kind": "prove", "curve": curve, "log_n": logn, "reps": reps, "device": new.info()["name"].strip(), "tables": lay["tables"],
           "wire_indexed": lay["wire_indexed"], "counts": rows}
    new.close()
    par.close()
    print(TAG + json.dumps(res), flush=True)


def run_compute_h(curve, logn, reps, parent_lib, count=16):
    import numpy as np
    from gnark_amd import fft, synth
    from gnark_amd.device import curve_id
    new, par = contexts(parent_lib)
    cid, n = curve_id(curve), 1 << logn
    A, B, Cc = (np.stack([synth._gen_scalars(new, cid, n, 0xC0 + 3 * j + k) for j in range(count)]) for k in range(3))
    d_new, d_par = fft.Domain(new, curve, n), fft.Domain(par, curve, n)
    try:
        batch = lambda: d_new.compute_h_batch(A, B, Cc)
        loop = lambda: [d_par.compute_h(A[j], B[j], Cc[j]) for j in range(count)]
        same = bool(np.array_equal(batch(), np.stack(loop())))
        (b_ms, l_ms), _ = interleaved(reps, [(new, batch), (par, loop)])
        stages = stage_profile(new, batch)
    finally:
        d_new.close()
        d_par.close()
    res = {"kind": "compute_h", "curve": curve, "log_n": logn, "count": count, "reps": reps, "batch_ms": round(b_ms, 4),
           "parent_sequential_ms": round(l_ms, 4), "speedup": round(l_ms / b_ms, 3), "equal": same,
           "batch_stages_ms": stages}
    new.close()
    par.close()
    print(TAG + json.dumps(res), flush=True)


def run_single(curve, logn, reps, parent_lib):
    from gnark_amd import groth16, synth
    new, par = contexts(parent_lib)
    inst = synth.make_instance(new, curve, logn, want_dlogs=False)
    pk_new, pk_par = inst.proving_key(new, precompute=1), inst.proving_key(par, precompute=1)
    try:
        one = lambda pk: (lambda: groth16.Prove(pk, inst.solution, inst.nb_public, inst.r, inst.s))
        same = one(pk_new)().raw().tobytes() == one(pk_par)().raw().tobytes()
        (n_ms, p_ms), (n_min, p_min) = interleaved(reps, [(new, one(pk_new)), (par, one(pk_par))])
    finally:
        pk_new.FreeGPUResources()
        pk_par.FreeGPUResources()
    res = {"kind": "single", "curve": curve, "log_n": logn, "reps": reps, "new_ms": round(n_ms, 4), "parent_ms": round(p_ms, 4),
           "new_over_parent": round(n_ms / p_ms, 4), "new_min_ms": round(n_min, 4), "parent_min_ms": round(p_min, 4), "proof_bytes_equal": same}
    new.close()
    par.close()
    print(TAG + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=3, metavar=("KIND", "CURVE", "LOGN"), help="(child) measure one configuration")
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "gnark_amd", "variants", "libgnark_amd_parent.so"))
    ap.add_argument("--log-n", type=int, nargs="+", default=[10, 12, 14, 16])
    ap.add_argument("--counts", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--compute-h-log-n", type=int, nargs="*", default=[10, 14])
    ap.add_argument("--single-log-n", type=int, nargs="*", default=[10, 20])
    ap.add_argument("--curves", nargs="+", default=list(CURVES))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prove_batch.json"))
    args = ap.parse_args()
    if not os.path.exists(args.parent_lib):
        sys.stderr.write("%s not found: build the parent commit's library first (see the top of this file)\n" % args.parent_lib)
        return 2
    if args.one:
        kind, curve, logn = args.one[0], args.one[1], int(args.one[2])
        if kind == "prove":
            run_prove(curve, logn, args.counts, args.reps, args.parent_lib)
        elif kind == "compute_h":
            run_compute_h(curve, logn, args.reps, args.parent_lib)
        else:
            run_single(curve, logn, args.reps, args.parent_lib)
        return 0
    steps = [("prove", cv, ln) for ln in args.log_n for cv in args.curves]
    steps += [("compute_h", cv, ln) for ln in args.compute_h_log_n for cv in args.curves]
    steps += [("single", "bn254", ln) for ln in args.single_log_n]
    results = []
    for kind, curve, logn in steps:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--one", kind, curve, str(logn),
               "--parent-lib", args.parent_lib, "--reps", str(args.reps), "--counts"] + [str(k) for k in args.counts]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
        if r.returncode != 0 or not line:   # a failed step ends the run: nothing more is started on the device
            sys.stderr.write("step %s failed (exit %d)\n%s\n%s\n" % ((kind, curve, logn), r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            return 1
        results.append(json.loads(line[0][len(TAG):]))
        print(line[0][:300], flush=True)
    prove = [r for r in results if r["kind"] == "prove"]
    floor = {"what": "count = 16, BN254, 2^10 and 2^12: the batch's time per proof is at most half the parent build's sequential time per proof"}
    for r in prove:
        if r["curve"] == "bn254" and r["log_n"] in (10, 12):
            for row in r["counts"]:
                if row["count"] == 16:
                    floor["2^%d" % r["log_n"]] = {"batch_ms_per_proof": row["batch_ms_per_proof"],
                                                  "parent_sequential_ms_per_proof": row["parent_sequential_ms_per_proof"], "met": row["speedup"] >= 2.0}
    doc = {"box": {"device": prove[0]["device"] if prove else None, "devices_used": 1},
           "method": "wall clock between ga_sync fences, median of `reps` interleaved repetitions after one warm-up; the baseline is a loop of "
                     "ga_g16_prove on a library built from the parent commit, loaded into the same process; keys pinned with precompute = 1",
           "prove_batch": prove, "compute_h_batch": [r for r in results if r["kind"] == "compute_h"],
           "single_proof_sanity": [r for r in results if r["kind"] == "single"], "done_criterion": floor}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

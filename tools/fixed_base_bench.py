#!/usr/bin/env python3
"""Times ga_batch_scalar_mul (fixed-base batch scalar multiplication, gnark_amd/csrc/fixed_base.hip.h) on the device and writes
profiles/fixed_base.json.

    python tools/fixed_base_bench.py [--log-n 20 24] [--reps 3] [--bench-json FILE] [--out profiles/fixed_base.json]

Every configuration (BN254 G1, BN254 G2, BLS12-381 G1 at each size) runs in a child process of its own under `timeout`; the first
child that fails ends the run.  Scalars and output are on the device, the table build is included in `total_ms`, and the three
stages are given separately from the hipEvents of the stage profiler.  Beside the device figures the file records
  * the bucket kernel's addition rate, when --bench-json names the detail file of a `python bench.py` run on the same box
    (its msm_accumulate stage: windows x n additions per launch), and
  * the time of oracle.generator_mul looped over 2^12 scalars on one CPU core -- the plain-C port of the test oracle, the only CPU
    figure this repository can produce; it is not gnark-crypto's BatchScalarMultiplication and the ratio is not a claim."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = [("bn254", 0), ("bn254", 1), ("bls12-381", 0)]
STAGES = ("fixed_base_table", "fixed_base_accumulate", "fixed_base_affine")


def run_one(curve, group, logn, reps):
    import numpy as np

    import gnark_amd
    import pyref
    from gnark_amd import _lib, ecc
    from gnark_amd.device import affine_words, curve_id
    from helpers import gen_of, pts_to_arr

    cid, n = curve_id(curve), 1 << logn
    c = pyref.BN254 if cid == 0 else pyref.BLS12_381
    base = pts_to_arr(c, group, [gen_of(c, group)])
    with gnark_amd.Context(0) as ctx:
        lib = ctx.lib
        s, out = ctx.malloc(n * 32), ctx.malloc(n * affine_words(cid, group) * 8)
        lib.check(lib.ga_gen_scalars(ctx.handle, cid, 0xF1BE + logn, n, s.ptr))
        flags = _lib.SCALARS_ON_DEVICE | _lib.RESULT_ON_DEVICE

        def call():
            lib.check(lib.ga_batch_scalar_mul(ctx.handle, cid, group, base.ctypes.data_as(C.c_void_p), C.c_void_p(s.ptr), n, flags, C.c_void_p(out.ptr)))

        call()   # warm-up: the scratch exists afterwards
        ctx.profile(True)
        ctx.profile_reset()
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        wall = (time.perf_counter() - t0) / reps * 1e3
        st = {}
        for name, ms in ctx.profile_read():
            st[name] = st.get(name, 0.0) + ms / reps
        ctx.profile(False)
        first = out.to_host((1, affine_words(cid, group)))
        s.free()
        out.free()
    cw, nwin = ecc.batch_scalar_mul_plan(curve, n, lib=lib)   # the width the library used
    windows = (cw, nwin)
    res = {"curve": curve, "group": "G%d" % (group + 1), "log_n": logn, "reps": reps, "window_bits": windows[0], "windows": windows[1],
           "wall_ms": round(wall, 3), "total_ms": round(sum(st.get(k, 0.0) for k in STAGES), 3),
           "stages_ms": {k: round(st.get(k, 0.0), 3) for k in STAGES}, "nonzero_output": bool(first.any())}
    acc = st.get("fixed_base_accumulate")
    if acc:
        res["accumulate_additions_per_s"] = round(windows[1] * n / (acc * 1e-3))
    res["points_per_s"] = round(n / (res["total_ms"] * 1e-3)) if res["total_ms"] else None
    print("FIXED_BASE_RESULT " + json.dumps(res), flush=True)


def bucket_rate(path):
    """additions per second of the MSM's bucket kernel from the detail file of a bench.py run (--detail-file): the headline leg's
    stages_ms.msm_accumulate.avg_ms and roofline.int_additions_per_launch (= config.windows x points per launch)"""
    with open(path) as f:
        doc = json.load(f)
    try:
        ms = doc["stages_ms"]["msm_accumulate"]["avg_ms"]
        adds = doc["roofline"]["int_additions_per_launch"]
        windows = doc["config"]["windows"]
    except (KeyError, TypeError) as e:
        raise SystemExit("%s: not a bench.py detail file with the headline MSM's stages (%r missing)" % (path, e))
    if not ms or not adds:
        raise SystemExit("%s: msm_accumulate was not timed in that run" % path)
    return {"msm_accumulate_ms": ms, "windows": windows, "additions": adds, "additions_per_s": round(adds / (ms * 1e-3)),
            "metric": doc.get("metric"), "ms_per_step": doc.get("ms_per_step")}


def cpu_reference(count=1 << 12):
    import oracle
    import pyref
    out = {}
    for c in (pyref.BN254, pyref.BLS12_381):
        rng = pyref.Xoshiro(0xC9C9)
        ks = [rng.field(c.r) for _ in range(count)]
        for group in (0, 1):
            if (c.name, group) not in CONFIGS:
                continue
            t0 = time.perf_counter()
            for k in ks:
                oracle.generator_mul(c.cid, group, k)
            dt = time.perf_counter() - t0
            out["%s_G%d" % (c.name, group + 1)] = {"scalars": count, "seconds": round(dt, 4), "points_per_s": round(count / dt)}
    return {"what": "oracle.generator_mul (the test oracle's plain-C double-and-add port) looped on one core; NOT gnark-crypto", "results": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=3, metavar=("CURVE", "GROUP", "LOGN"), help="(child) measure one configuration")
    ap.add_argument("--log-n", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--bench-json", default="", help="detail file of a bench.py run on the same box (bucket kernel rate)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fixed_base.json"))
    args = ap.parse_args()
    if args.one:
        run_one(args.one[0], int(args.one[1]), int(args.one[2]), args.reps)
        return 0
    bucket = bucket_rate(args.bench_json) if args.bench_json else None   # (fails before anything is started on the device)
    results = []
    for logn in args.log_n:
        for curve, group in CONFIGS:
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--one", curve, str(group), str(logn),
                   "--reps", str(args.reps)]
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("FIXED_BASE_RESULT ")]
            if r.returncode != 0 or not line:   # a failed step ends the run: nothing more is started on the device
                sys.stderr.write("step %s failed (exit %d)\n%s\n%s\n" % (cmd[5:], r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
                return 1
            results.append(json.loads(line[0][len("FIXED_BASE_RESULT "):]))
            print(line[0], flush=True)
    doc = {"device_results": results, "bucket_kernel": bucket, "cpu_reference": cpu_reference()}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

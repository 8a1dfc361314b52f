#!/usr/bin/env python3
"""Times ga_kzg_to_lagrange_g1 (kzg.ToLagrangeG1: the inverse FFT over G1 points, gnark_amd/csrc/ec_ntt.hip.h) on the device and
writes profiles/to_lagrange.json.

    python tools/to_lagrange_bench.py [--log-n 16 20 22] [--reps 2] [--out profiles/to_lagrange.json]

Every configuration (BN254, BLS12-381 at each size) runs in a child process of its own under `timeout`; the first child that
fails ends the run.  Input and output are on the device; the times are the hipEvents of the stage profiler around every kernel of
the call, after one warm-up call.  Per configuration the file records
  * the time of every stage and the point operations it needs (doublings and additions of the double-and-add loops, counted from
    the scalars themselves, plus the two additions of every butterfly), hence the achieved point operations per second;
  * the yardstick, measured in the same process: the mixed-addition rate of ga_batch_scalar_mul's accumulation kernel at the same n;
  * the A/B of the lane order (GA_EC_NTT_UNIFORM=0: consecutive butterflies of one group in a wave at every stage), same process.
There is no CPU figure: gnark-crypto is not available to this repository, and none is made up."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

CURVES = ("bn254", "bls12-381")


def stage_ops(c, logn):
    """(doublings, additions) every stage needs, from its scalars: a scalar k costs bit_length(k) - 1 doublings and popcount(k) - 1
    additions; every butterfly adds twice (a + b, a - b)"""
    import numpy as np
    n, r = 1 << logn, c.r
    half = n // 2
    winv, ninv = pow(c.fr_root_of_unity(n), -1, r), pow(n, -1, r)
    bl, pc = np.zeros(half, np.int64), np.zeros(half, np.int64)
    bl0, pc0 = np.zeros(half, np.int64), np.zeros(half, np.int64)   # the same twiddles times 1/n (group 0 of every stage)
    t = 1
    for j in range(half):
        k0 = t * ninv % r
        bl[j], pc[j], bl0[j], pc0[j] = t.bit_length(), bin(t).count("1"), k0.bit_length(), bin(k0).count("1")
        t = t * winv % r
    out = []
    for s in range(logn):
        groups = 1 << s
        sel = slice(0, half, groups)   # tw[j << s], j < m
        dbl = int((bl0[sel] - 1).sum()) + (groups - 1) * int((bl[sel][1:] - 1).sum())
        add = int((pc0[sel] - 1).sum()) + (groups - 1) * int((pc[sel][1:] - 1).sum())
        out.append((dbl, add + 2 * half))
    return out


def run_one(curve, logn, reps):
    import gnark_amd
    import pyref
    from gnark_amd import _lib, ecc
    from gnark_amd.device import affine_words, curve_id
    from helpers import gen_of, pts_to_arr

    cid, n = curve_id(curve), 1 << logn
    c = pyref.BN254 if cid == 0 else pyref.BLS12_381
    wa = affine_words(cid, 0)
    base = pts_to_arr(c, 0, [gen_of(c, 0)])
    ops = stage_ops(c, logn)
    with gnark_amd.Context(0) as ctx:
        lib = ctx.lib
        s, pts, out = ctx.malloc(n * 32), ctx.malloc(n * wa * 8), ctx.malloc(n * wa * 8)
        lib.check(lib.ga_gen_scalars(ctx.handle, cid, 0x7A6 + logn, n, s.ptr))

        def fixed_base():   # the input points: n random multiples of the generator -- and the yardstick
            lib.check(lib.ga_batch_scalar_mul(ctx.handle, cid, 0, base.ctypes.data_as(C.c_void_p), C.c_void_p(s.ptr), n,
                                              _lib.SCALARS_ON_DEVICE | _lib.RESULT_ON_DEVICE, C.c_void_p(pts.ptr)))

        def to_lagrange():
            lib.check(lib.ga_kzg_to_lagrange_g1(ctx.handle, cid, C.c_void_p(pts.ptr), n, _lib.BASES_ON_DEVICE | _lib.RESULT_ON_DEVICE, C.c_void_p(out.ptr)))

        def timed(call):
            ctx.profile(True)
            ctx.profile_reset()
            for _ in range(reps):
                call()
            st = {}
            for name, ms in ctx.profile_read():
                st[name] = st.get(name, 0.0) + ms / reps
            ctx.profile(False)
            return st

        fixed_base()   # warm-up of both entry points: the scratch exists afterwards
        to_lagrange()
        fb = timed(fixed_base)
        st = timed(to_lagrange)
        os.environ["GA_EC_NTT_UNIFORM"] = "0"
        to_lagrange()
        st0 = timed(to_lagrange)
        del os.environ["GA_EC_NTT_UNIFORM"]
        first = out.to_host((1, wa))
        for b in (s, pts, out):
            b.free()
    nwin = ecc.batch_scalar_mul_plan(curve, n, lib=lib)[1]
    stage_ms = [st.get("ec_ntt_stage_%02d" % k, 0.0) for k in range(logn)]
    stage_ms0 = [st0.get("ec_ntt_stage_%02d" % k, 0.0) for k in range(logn)]
    total_ops = sum(d + a for d, a in ops)
    stages_total = sum(stage_ms)
    yard = nwin * n / (fb["fixed_base_accumulate"] * 1e-3)
    res = {"curve": curve, "log_n": logn, "reps": reps, "total_ms": round(sum(st.values()), 3), "stages_total_ms": round(stages_total, 3),
           "other_ms": {k: round(v, 3) for k, v in st.items() if not k.startswith("ec_ntt_stage_")},
           "stages": [{"stage": k, "ms": round(stage_ms[k], 3), "doublings": ops[k][0], "additions": ops[k][1],
                       "point_ops_per_s": round((ops[k][0] + ops[k][1]) / (stage_ms[k] * 1e-3)) if stage_ms[k] else None} for k in range(logn)],
           "doublings": sum(d for d, _ in ops), "additions": sum(a for _, a in ops),
           "point_ops_per_s": round(total_ops / (stages_total * 1e-3)),
           "yardstick": {"what": "ga_batch_scalar_mul accumulation kernel (lazy mixed additions, 10 products each), same process, same n",
                         "fixed_base_accumulate_ms": round(fb["fixed_base_accumulate"], 3), "windows": nwin, "additions_per_s": round(yard)},
           "point_ops_per_s_over_yardstick": round(total_ops / (stages_total * 1e-3) / yard, 4),
           "ab_lane_order": {"what": "GA_EC_NTT_UNIFORM=0: a wave holds consecutive butterflies of one group at every stage (the simpler "
                                     "order); default: from stage 6 on the lanes of a wave share their scalar",
                             "uniform_stages_total_ms": round(stages_total, 3), "consecutive_stages_total_ms": round(sum(stage_ms0), 3),
                             "consecutive_stage_ms": [round(v, 3) for v in stage_ms0]},
           "nonzero_output": bool(first.any())}
    print("TO_LAGRANGE_RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=2, metavar=("CURVE", "LOGN"), help="(child) measure one configuration")
    ap.add_argument("--log-n", type=int, nargs="+", default=[16, 20, 22])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "to_lagrange.json"))
    args = ap.parse_args()
    if args.one:
        run_one(args.one[0], int(args.one[1]), args.reps)
        return 0
    results = []
    for logn in args.log_n:
        for curve in CURVES:
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--one", curve, str(logn), "--reps", str(args.reps)]
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("TO_LAGRANGE_RESULT ")]
            if r.returncode != 0 or not line:   # a failed step ends the run: nothing more is started on the device
                sys.stderr.write("step %s failed (exit %d)\n%s\n%s\n" % (cmd[5:], r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
                return 1
            results.append(json.loads(line[0][len("TO_LAGRANGE_RESULT "):]))
            print(line[0][:400], flush=True)
    doc = {"device_results": results,
           "cpu_reference": None, "cpu_reference_note": "gnark-crypto's kzg.ToLagrangeG1 was not available where this was measured: no CPU figure"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

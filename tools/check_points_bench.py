#!/usr/bin/env python3
"""Times ga_check_points (batch curve and subgroup checks, gnark_amd/csrc/check_points.hip.h) and the checked key reads on the device
and writes profiles/check_points.json.

    python tools/check_points_bench.py [--log-n 16 20] [--g2-log-n 16 18] [--reps 3] [--curves bn254 bls12-381] [--key-log-n 20] [--out profiles/check_points.json]

One process.  The points are on the device and no status is asked for; the times are the hipEvents of the stage profiler around the
kernels of a call.  Per curve and group and size the fast test (the identity in the curve's seed) and GA_CHECK_NAIVE=1 ([r - 1]P = -P
on the plain ladder) run once warm and then `reps` times each, interleaved call by call; the file records the milliseconds of every
call, points per second, the counts every call returned, and the measured fast / naive ratio beside the predicted one -- from 9
products a doubling and 14 an addition applied to the bits of |x0| and of r - 1.  The fast test "wins" a group when its slowest call
beats the naive test's fastest.  The yardstick, in the same process on the same points: the plain ladder of ga_scale_points
(GA_SCALE_WINDOW=0) with full-width scalars.  Then, per curve, one synthetic key of 2^key-log-n constraints written in the three
layouts and read back unchecked and checked (wall clock, no window tables).
There is no CPU figure: gnark-crypto is not available to this repository, and none is made up."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

CURVES = ("bn254", "bls12-381")
SEED = {"bn254": 4965661367192848881, "bls12-381": 0xd201000000010000}
PREDICTED = {("bls12-381", 0): 0.31, ("bls12-381", 1): 0.16, ("bn254", 1): 0.27}   # fast / naive; BN254 G1 has no ladder to predict


def ladder_products(k):
    """field products of left-to-right double-and-add by k: 9 a doubling, 14 an addition"""
    return 9 * (k.bit_length() - 1) + 14 * (bin(k).count("1") - 1)


def model_ratio(curve, group, r):
    if (curve, group) == ("bn254", 0):
        return None
    fast = ladder_products(SEED[curve]) * (2 if (curve, group) == ("bls12-381", 0) else 1)
    return round(fast / ladder_products(r - 1), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--g2-log-n", type=int, nargs="+", default=[16, 18])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--curves", nargs="+", default=list(CURVES))
    ap.add_argument("--key-log-n", type=int, default=20, help="0 skips the key reads")
    ap.add_argument("--dir", default=tempfile.gettempdir())
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "check_points.json"))
    args = ap.parse_args()

    import gnark_amd
    import pyref
    from gnark_amd import _lib, groth16, synth
    from gnark_amd.device import affine_words, curve_id
    from helpers import gen_of, pts_to_arr

    results, keys = [], []
    with gnark_amd.Context(0) as ctx:
        lib = ctx.lib

        def profiled(call):
            ctx.profile(True)
            ctx.profile_reset()
            ret = call()
            st = {}
            for name, ms in ctx.profile_read():
                st[name] = st.get(name, 0.0) + ms
            ctx.profile(False)
            return st, ret

        for curve in args.curves:
            cid = curve_id(curve)
            c = pyref.BN254 if cid == 0 else pyref.BLS12_381
            for group, logn in [(0, ln) for ln in args.log_n] + [(1, ln) for ln in args.g2_log_n]:
                n, wa = 1 << logn, affine_words(cid, group)
                rng = np.random.default_rng(0xC4EC + 1000 * cid + 10 * logn + group)

                def rand_words(m):   # full-width scalars below r: the top word below r's
                    w = rng.integers(0, 1 << 64, size=(m, 4), dtype=np.uint64)
                    w[:, 3] = rng.integers(1, c.r >> 192, size=m, dtype=np.uint64)
                    return w
                base = pts_to_arr(c, group, [gen_of(c, group)])
                logs, pts, out, d_s = ctx.to_device(rand_words(n)), ctx.malloc(n * wa * 8), ctx.malloc(n * wa * 8), ctx.to_device(rand_words(n))
                lib.check(lib.ga_batch_scalar_mul(ctx.handle, cid, group, base.ctypes.data_as(C.c_void_p), C.c_void_p(logs.ptr), n,
                                                  _lib.SCALARS_ON_DEVICE | _lib.RESULT_ON_DEVICE, C.c_void_p(pts.ptr)))

                def check():
                    out4 = (C.c_uint64 * 4)()
                    lib.check(lib.ga_check_points(ctx.handle, cid, group, C.c_void_p(pts.ptr), n, _lib.BASES_ON_DEVICE, None, out4))
                    return list(out4)

                def scale():
                    red = C.c_uint64(0)
                    lib.check(lib.ga_scale_points(ctx.handle, cid, group, C.c_void_p(pts.ptr), n, _lib.SCALE_EACH, C.c_void_p(d_s.ptr), 0,
                                                  _lib.SCALARS_ON_DEVICE | _lib.BASES_ON_DEVICE | _lib.RESULT_ON_DEVICE, C.c_void_p(out.ptr), C.byref(red)))
                    return red.value

                runs = {"fast": [], "naive": [], "scale_plain": []}
                for rep in range(args.reps + 1):   # (rep 0 warms all three up: the scratch exists afterwards)
                    for name, env in (("fast", None), ("naive", "1")):
                        if env is None:
                            os.environ.pop("GA_CHECK_NAIVE", None)
                        else:
                            os.environ["GA_CHECK_NAIVE"] = env
                        st, out4 = profiled(check)
                        if rep:
                            runs[name].append((st["check_ladder"], out4))
                    os.environ.pop("GA_CHECK_NAIVE", None)
                    os.environ["GA_SCALE_WINDOW"] = "0"
                    st, redone = profiled(scale)
                    os.environ.pop("GA_SCALE_WINDOW", None)
                    if rep:
                        runs["scale_plain"].append((st["scale_ladder"], redone))
                rec = {"curve": curve, "group": "G2" if group else "G1", "log_n": logn, "reps": args.reps}
                for name in ("fast", "naive"):
                    ms = [v for v, _ in runs[name]]
                    assert all(o == [0, 0, (1 << 64) - 1, 0] for _, o in runs[name]), runs[name]
                    rec[name] = {"ms": [round(v, 3) for v in ms], "points_per_s": round(n / (min(ms) * 1e-3)), "out4": runs[name][0][1]}
                sp = [v for v, _ in runs["scale_plain"]]
                rec["scale_points_plain_ladder"] = {"ms": [round(v, 3) for v in sp], "points_per_s": round(n / (min(sp) * 1e-3))}
                f, nv = rec["fast"]["ms"], rec["naive"]["ms"]
                rec["fast_over_naive"] = round(min(f) / min(nv), 4)
                rec["predicted_fast_over_naive"] = PREDICTED.get((curve, group))
                rec["product_count_ratio"] = model_ratio(curve, group, c.r)
                rec["naive_over_scale_points_plain"] = round(min(nv) / min(sp), 4)
                rec["fast_wins_beyond_spread"] = bool(max(f) < min(nv))
                results.append(rec)
                print("CHECK_POINTS_RESULT " + json.dumps({k: rec[k] for k in ("curve", "group", "log_n", "fast_over_naive", "predicted_fast_over_naive",
                                                                                "fast_wins_beyond_spread")}) + " fast %s naive %s scale %s" % (f, nv, rec["scale_points_plain_ladder"]["ms"]),
                      flush=True)
                for b in (logs, pts, out, d_s):
                    b.free()

            if args.key_log_n:   # one synthetic key, three layouts, unchecked and checked
                inst = synth.make_instance(ctx, curve, args.key_log_n, 0xF11E, want_dlogs=False)
                for fmt, name in ((groth16.KEY_FORMAT_COMPRESSED, "WriteTo (compressed)"), (groth16.KEY_FORMAT_RAW, "WriteRawTo"), (groth16.KEY_FORMAT_DUMP, "WriteDump")):
                    path = os.path.join(args.dir, "ga_check_key_%d_%d.bin" % (os.getpid(), fmt))
                    rec = {"curve": curve, "log_n": args.key_log_n, "format": name}
                    try:
                        with open(path, "wb") as f:
                            size = groth16.WriteKey(ctx, curve, f, fmt, domain_cardinality=inst.n, **inst.key)
                        rec["file_mib"] = round(size / 2**20, 1)
                        for rep in range(2):   # (the first pass warms the page cache and the scratch)
                            for check, tag in ((False, "read_unchecked_s"), (True, "read_checked_s")):
                                t0 = time.perf_counter()
                                with open(path, "rb") as f:
                                    pk = groth16.ProvingKey.ReadFrom(ctx, curve, f, precompute=-1, subgroup_check=check)
                                ctx.sync()
                                rec[tag] = round(time.perf_counter() - t0, 3)
                                pk.FreeGPUResources()
                        rec["checked_over_unchecked"] = round(rec["read_checked_s"] / rec["read_unchecked_s"], 3)
                    finally:
                        if os.path.exists(path):
                            os.unlink(path)
                    keys.append(rec)
                    print("CHECK_POINTS_KEY " + json.dumps(rec), flush=True)
    doc = {"device_results": results, "key_reads": keys,
           "predicted_note": "fast / naive predicted from 9 field products a doubling and 14 an addition on the bits of |x0| and of r - 1; product_count_ratio is "
                             "that model recomputed here, predicted_fast_over_naive the figure written down before anything was measured",
           "cpu_reference": None, "cpu_reference_note": "gnark-crypto was not available where this was measured: no CPU figure"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

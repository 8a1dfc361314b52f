#!/usr/bin/env python3
"""Times ga_scale_points (per-point scalar multiplication, gnark_amd/csrc/scale_points.hip.h: the curve work of the Groth16 MPC
ceremony) on the device and writes profiles/scale_points.json.

    python tools/scale_points_bench.py [--log-n 16 20] [--g2-log-n 16] [--reps 3] [--out profiles/scale_points.json]

One process.  Points, scalars and output are on the device; the times are the hipEvents of the stage profiler around every kernel of
a call.  Every configuration -- BN254 and BLS12-381, G1 at every size in the three modes, G2 in GA_SCALE_POWERS -- runs once warm
and then `reps` times with the signed 4-bit windows and `reps` times with GA_SCALE_WINDOW=0 (the plain double-and-add ladder),
interleaved call by call.  Per run the file records the milliseconds of every call, multiplications per second, `redone`, and the
point operations per second counted from the digits (windowed: the table's 4 doublings + 3 additions, 4 doublings per window below
the top digit, one addition per non-zero digit) or bits (plain: one doubling per bit below the top one, one addition per set bit) of
the scalars themselves -- per lane, and per wave (a wave executes an addition when ANY of its 64 lanes needs it).  The windowed
ladder "wins" a configuration when its slowest call beats the plain ladder's fastest.  The yardstick, measured in the same process:
the mixed-addition rate of ga_batch_scalar_mul's accumulation kernel, which also makes the input points.
There is no CPU figure: gnark-crypto is not available to this repository, and none is made up."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

CURVES = ("bn254", "bls12-381")
MODES = ("each", "one", "powers")
PREDICTED = {"each": 0.55, "powers": 0.55, "one": 0.80}   # windowed / plain, from 9 products a doubling and 14 an addition


def to_words(ks):
    return np.frombuffer(b"".join(int(k).to_bytes(32, "little") for k in ks), dtype=np.uint64).reshape(-1, 4).copy()


def op_counts(words):
    """(n, 4) canonical scalars -> per-lane and per-wave doublings and additions of both ladders"""
    n = words.shape[0]
    by = words.view(np.uint8).reshape(n, 32)
    nib = np.empty((n, 65), np.int16)
    nib[:, 0:64:2], nib[:, 1:64:2], nib[:, 64] = by & 15, by >> 4, 0
    carry = np.zeros(n, np.int16)
    for w in range(65):   # digits in [-8, 8]
        d = nib[:, w] + carry
        carry = (d > 8).astype(np.int16)
        nib[:, w] = d - 16 * carry
    nz = nib != 0
    live = nz.any(axis=1)
    top = np.where(live, 64 - np.argmax(nz[:, ::-1], axis=1), 0)
    w_dbl = 4 * top + 4 * live
    w_add = nz.sum(axis=1) - live + 3 * live
    bits = np.unpackbits(by, axis=1, bitorder="little")
    btop = np.where(live, 255 - np.argmax(bits[:, ::-1], axis=1), 0)
    p_dbl, p_add = btop, bits.sum(axis=1) - live
    pad = (-n) % 64

    def wave(per_lane_top, mask):   # a wave runs to its highest top and adds wherever any lane adds
        t = np.pad(per_lane_top, (0, pad)).reshape(-1, 64).max(axis=1)
        m = np.pad(mask, ((0, pad), (0, 0))).reshape(-1, 64, mask.shape[1]).any(axis=1)
        return t, m.sum(axis=1)
    wt, wa = wave(top, nz)
    bt, ba = wave(btop, bits.astype(bool))
    return {"window": {"lane_doublings": int(w_dbl.sum()), "lane_additions": int(w_add.sum()),
                       "wave_doublings": int((4 * wt + 4).sum()) * 64, "wave_additions": int((wa - 1 + 3).sum()) * 64},
            "plain": {"lane_doublings": int(p_dbl.sum()), "lane_additions": int(p_add.sum()),
                      "wave_doublings": int(bt.sum()) * 64, "wave_additions": int((ba - 1).sum()) * 64}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--g2-log-n", type=int, nargs="+", default=[16])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scale_points.json"))
    args = ap.parse_args()

    import gnark_amd
    import pyref
    from gnark_amd import _lib, ecc
    from gnark_amd.device import affine_words, curve_id
    from helpers import gen_of, pts_to_arr

    results, yard = [], []
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

        for curve in CURVES:
            cid = curve_id(curve)
            c = pyref.BN254 if cid == 0 else pyref.BLS12_381
            for group, logn, modes in [(0, ln, MODES) for ln in args.log_n] + [(1, ln, ("powers",)) for ln in args.g2_log_n]:
                n, wa = 1 << logn, affine_words(cid, group)
                rng = np.random.default_rng(0x5CA1E + 1000 * cid + logn)
                rtop = c.r >> 192

                def rand_words(m):   # full-width scalars below r: the top word below r's
                    w = rng.integers(0, 1 << 64, size=(m, 4), dtype=np.uint64)
                    w[:, 3] = rng.integers(1, rtop, size=m, dtype=np.uint64)
                    return w
                base = pts_to_arr(c, group, [gen_of(c, group)])
                logs, pts, out = ctx.to_device(rand_words(n)), ctx.malloc(n * wa * 8), ctx.malloc(n * wa * 8)

                def make_points():   # the input: n random multiples of the generator -- and, for G1, the yardstick
                    lib.check(lib.ga_batch_scalar_mul(ctx.handle, cid, group, base.ctypes.data_as(C.c_void_p), C.c_void_p(logs.ptr), n,
                                                      _lib.SCALARS_ON_DEVICE | _lib.RESULT_ON_DEVICE, C.c_void_p(pts.ptr)))
                make_points()
                fb, _ = profiled(make_points)
                nwin = ecc.batch_scalar_mul_plan(curve, n, lib=lib)[1]
                yard_rate = nwin * n / (fb["fixed_base_accumulate"] * 1e-3)
                if group == 0:
                    yard.append({"curve": curve, "log_n": logn, "fixed_base_accumulate_ms": round(fb["fixed_base_accumulate"], 3), "windows": nwin,
                                 "additions_per_s": round(yard_rate)})
                for mode in modes:
                    to_int = lambda row: sum(int(v) << (64 * k) for k, v in enumerate(row))
                    d_s = None
                    if mode == "each":
                        words = rand_words(n)
                        d_s = ctx.to_device(words)
                        kw = dict(scalars=d_s)
                    elif mode == "one":
                        s = to_int(rand_words(1)[0])
                        words, kw = np.repeat(to_words([s]), n, axis=0), dict(scalar=s)
                    else:
                        cc, t = (to_int(row) for row in rand_words(2))
                        ks, k = [], cc
                        for _ in range(n):
                            ks.append(k)
                            k = k * t % c.r
                        words, kw = to_words(ks), dict(powers=(cc, t))
                    ops = op_counts(words)

                    def call(kw=kw, d_s=d_s):   # (straight through the library: ecc.ScalePoints would allocate the output)
                        red = C.c_uint64(0)
                        if "scalars" in kw:
                            m, sp, fl = _lib.SCALE_EACH, C.c_void_p(d_s.ptr), _lib.SCALARS_ON_DEVICE
                        elif "scalar" in kw:
                            keep = to_words([kw["scalar"]])
                            m, sp, fl = _lib.SCALE_ONE, keep.ctypes.data_as(C.c_void_p), 0
                        else:
                            keep = to_words(kw["powers"])
                            m, sp, fl = _lib.SCALE_POWERS, keep.ctypes.data_as(C.c_void_p), 0
                        lib.check(lib.ga_scale_points(ctx.handle, cid, group, C.c_void_p(pts.ptr), n, m, sp, 0,
                                                      fl | _lib.BASES_ON_DEVICE | _lib.RESULT_ON_DEVICE, C.c_void_p(out.ptr), C.byref(red)))
                        return red.value

                    runs = {"window": [], "plain": []}
                    for rep in range(args.reps + 1):   # (rep 0 warms both up: the scratch exists afterwards)
                        for name, env in (("window", None), ("plain", "0")):
                            if env is None:
                                os.environ.pop("GA_SCALE_WINDOW", None)
                            else:
                                os.environ["GA_SCALE_WINDOW"] = env
                            st, redone = profiled(call)
                            if rep:
                                runs[name].append((st, redone))
                    os.environ.pop("GA_SCALE_WINDOW", None)
                    rec = {"curve": curve, "group": "G2" if group else "G1", "log_n": logn, "mode": mode, "reps": args.reps}
                    for name, rr in runs.items():
                        ladder = [st["scale_ladder"] for st, _ in rr]
                        total = [sum(st.values()) for st, _ in rr]
                        best = min(ladder)
                        o = ops[name]
                        rec[name] = {"ladder_ms": [round(v, 3) for v in ladder], "total_ms": [round(v, 3) for v in total],
                                     "other_ms": {k: round(v, 3) for k, v in rr[0][0].items() if k != "scale_ladder"},
                                     "redone": [rd for _, rd in rr], "multiplications_per_s": round(n / (min(total) * 1e-3)), **o,
                                     "lane_point_ops_per_s": round((o["lane_doublings"] + o["lane_additions"]) / (best * 1e-3)),
                                     "wave_point_ops_per_s": round((o["wave_doublings"] + o["wave_additions"]) / (best * 1e-3)),
                                     "lane_point_ops_per_s_over_yardstick": round((o["lane_doublings"] + o["lane_additions"]) / (best * 1e-3) / yard_rate, 4)}
                    w, p = rec["window"]["ladder_ms"], rec["plain"]["ladder_ms"]
                    rec["window_over_plain"] = round(min(w) / min(p), 4)
                    rec["predicted_window_over_plain"] = PREDICTED[mode]
                    rec["window_wins_beyond_spread"] = bool(max(w) < min(p))
                    results.append(rec)
                    print("SCALE_POINTS_RESULT " + json.dumps({k: rec[k] for k in ("curve", "group", "log_n", "mode", "window_over_plain", "window_wins_beyond_spread")})
                          + " window %s plain %s redone %s" % (w, p, rec["window"]["redone"]), flush=True)
                    if d_s is not None:
                        d_s.free()
                for b in (logs, pts, out):
                    b.free()
    doc = {"device_results": results,
           "yardstick": {"what": "ga_batch_scalar_mul accumulation kernel (lazy mixed additions, 10 products each), same process, same n", "runs": yard},
           "cpu_reference": None, "cpu_reference_note": "gnark-crypto's mpcsetup was not available where this was measured: no CPU figure"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

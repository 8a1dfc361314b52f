#!/usr/bin/env python3
"""Times the G1 / Fr calls on BLS12-377 against the same calls on BLS12-381 and writes profiles/bls12_377.json.

    python tools/bls12_377_bench.py [--reps 10] [--items msm:20 msm:22 fft:22 plonk:20] [--out profiles/bls12_377.json]

BLS12-381 is the yardstick: the same limb counts (14 x 28 bits for Fp, 9 x 29 for Fr), the same kernels, and two more scalar bits.
The expectation is therefore a ratio bls12-377 / bls12-381 at or below 1; the margin is the run-to-run spread of the BLS12-381
repetitions of the same run, (max - min) / median, recorded beside every figure.  A ratio above 1 + spread is reported in `findings`.

Items, each in a child process of its own under `timeout` (the first child that fails ends the run); both curves live in that one
process on one context and their timed runs are interleaved, 377, 381, 377, ...:
  msm:K    sum s_i P_i over 2^K synthetic G1 points (ga_gen_bases, ga_gen_scalars), bases and scalars in device memory:
           `msm` = ga_msm on the plain bases, `table` = ga_msm_table_run on a window table
  fft:K    one forward DIF ga_fft of 2^K elements in device memory
  plonk:K  grand product + quotient over a pinned key (nb_bsb = 1) + one opening over an SRS table, n = 2^K: ga_plonk_build_z,
           ga_plonk_quotient_pinned, ga_kzg_open, operands in device memory; the three calls timed separately, `sum` their total
A timed region starts and ends with ga_sync; the figure is the median wall-clock time of `reps` repetitions after one warm-up of each
side.  Window widths, window counts and table sizes are recorded: the two curves may be planned differently (253 against 255 bits);
so is one stage breakdown of each MSM from the stage profiler, taken in a separate pass."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW, REF = "bls12-377", "bls12-381"
TAG = "BLS12_377_RESULT "


def timed(ctx, call):
    ctx.sync()
    t0 = time.perf_counter()
    call()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3


def interleaved(ctx, reps, calls):
    """calls: {curve: call}; one warm-up each, then reps rounds of the curves in turn; {curve: [ms]}"""
    for call in calls.values():
        timed(ctx, call)
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, call in calls.items():
            ms[k].append(timed(ctx, call))
    return ms


def stage_profile(ctx, call):
    """one run under the stage profiler (hipEvent pairs around the named stages), in a pass of its own: {stage: ms}, largest first"""
    ctx.profile(True)
    ctx.profile_reset()
    call()
    st = {}
    for name, ms in ctx.profile_read():
        st[name] = st.get(name, 0.0) + ms
    ctx.profile_reset()
    ctx.profile(False)
    return {k: round(v, 4) for k, v in sorted(st.items(), key=lambda kv: -kv[1])}


def figure(ms):
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = (max(ms[REF]) - min(ms[REF])) / med[REF]
    ratio = med[NEW] / med[REF]
    return {"bls12_377_ms": round(med[NEW], 4), "bls12_381_ms": round(med[REF], 4), "ratio": round(ratio, 4), "bls12_381_spread": round(spread, 4),
            "bls12_377_min_ms": round(min(ms[NEW]), 4), "bls12_381_min_ms": round(min(ms[REF]), 4), "within_margin": bool(ratio <= 1 + spread)}


def run_msm(ctx, logn, reps):
    import numpy as np
    from gnark_amd import _lib, ecc
    from gnark_amd.device import affine_words, curve_id, jac_words
    n = 1 << logn
    calls_plain, calls_table, plans, keep = {}, {}, {}, []
    for curve in (NEW, REF):
        cid = curve_id(curve)
        bases, scal = ctx.malloc(n * affine_words(cid, 0) * 8), ctx.malloc(n * 32)
        ctx.lib.check(ctx.lib.ga_gen_bases(ctx.handle, cid, 0, 0xB377, n, bases.ptr, None))
        ctx.lib.check(ctx.lib.ga_gen_scalars(ctx.handle, cid, 0xC377, n, scal.ptr))
        table = ecc.PrecomputedBases(ctx, curve, 0, bases, n=n)
        out = np.zeros(jac_words(cid, 0), dtype=np.uint64)
        keep += [bases, scal, table, out]
        flags = _lib.BASES_ON_DEVICE | _lib.SCALARS_ON_DEVICE | _lib.SCALARS_MONTGOMERY
        calls_plain[curve] = lambda cid=cid, b=bases, s=scal, o=out: ctx.lib.check(
            ctx.lib.ga_msm(ctx.handle, cid, 0, b.ptr, s.ptr, n, flags, o.ctypes.data))
        calls_table[curve] = lambda t=table, s=scal, o=out: ctx.lib.check(
            ctx.lib.ga_msm_table_run(t.handle, s.ptr, _lib.SCALARS_ON_DEVICE | _lib.SCALARS_MONTGOMERY, o.ctypes.data))
        c, nw = ecc.plan(curve, 0, n, lib=ctx.lib)
        plans[curve] = {"msm_window_bits": c, "msm_windows": nw, **{"table_" + k: v for k, v in table.info().items()}}
    res = {"msm": figure(interleaved(ctx, reps, calls_plain)), "table": figure(interleaved(ctx, reps, calls_table)), "plans": plans}
    res["table_stages_ms"] = {curve: stage_profile(ctx, call) for curve, call in calls_table.items()}
    res["msm_stages_ms"] = {curve: stage_profile(ctx, call) for curve, call in calls_plain.items()}
    for k in keep:
        if hasattr(k, "free"):
            k.free()
    return res


def run_fft(ctx, logn, reps):
    from gnark_amd import _lib, fft
    from gnark_amd.device import curve_id
    n = 1 << logn
    calls, keep = {}, []
    for curve in (NEW, REF):
        d, buf = fft.Domain(ctx, curve, n), ctx.malloc(n * 32)
        ctx.lib.check(ctx.lib.ga_gen_scalars(ctx.handle, curve_id(curve), 0xF377, n, buf.ptr))
        keep += [d, buf]
        calls[curve] = lambda d=d, b=buf: ctx.lib.check(ctx.lib.ga_fft(d.handle, b.ptr, _lib.FFT_FORWARD, _lib.DIF, 0, 1))
    res = {"fft": figure(interleaved(ctx, reps, calls))}
    for d, buf in zip(keep[0::2], keep[1::2]):
        buf.free()
        d.close()
    return res


def run_plonk(ctx, logn, reps):
    import numpy as np
    from gnark_amd import _lib, ecc, fft, plonk, synth
    from gnark_amd.device import affine_words, curve_id, jac_words
    n = 1 << logn
    calls = {"build_z": {}, "quotient": {}, "open": {}}
    keep, plans = [], {}
    for curve in (NEW, REF):
        cid = curve_id(curve)
        gen = lambda count, seed: synth._gen_scalars(ctx, cid, count, seed)
        d0, d1 = fft.Domain(ctx, curve, n), fft.Domain(ctx, curve, plonk.Rho(n) * n)
        pk = plonk.ProvingKey(d0, d1, {k: gen(n, 0x920 + i) for i, k in enumerate(plonk.FIXED_IDS)}, [gen(n, 0x930)], lagrange=plonk.FIXED_IDS + ("Qcp0",))
        srs = ctx.malloc((n + 3) * affine_words(cid, 0) * 8)
        ctx.lib.check(ctx.lib.ga_gen_bases(ctx.handle, cid, 0, 0x960, n + 3, srs.ptr, None))
        table = ecc.PrecomputedBases(ctx, curve, 0, srs, n=n + 3)
        srs.free()
        bufs = {k: ctx.to_device(gen(n, 0x910 + i)) for i, k in enumerate(("l", "r", "o", "z", "qk", "pi2"))}
        bufs["perm"] = ctx.to_device(np.random.default_rng(0x940 + logn).permutation(3 * n).astype(np.int64))
        bufs["open"] = ctx.to_device(gen(n + 3, 0x950))
        z_out, h_out = ctx.malloc(n * 32), ctx.malloc(plonk.Rho(n) * n * 32)
        host = {k: gen(cnt, 0x970 + i) for i, (k, cnt) in enumerate((("bl", 2), ("br", 2), ("bo", 2), ("bz", 3), ("alpha", 1), ("beta", 1), ("gamma", 1), ("point", 1)))}
        a = _lib.PlonkQuotientIn()
        a.nb_bsb, a.flags = 1, 1   # GA_PLONK_ON_DEVICE
        a.lagrange_mask = sum(1 << k for k in (0, 1, 2, 3, 8, 13))   # L R O Z Qk Pi2_0 as evaluations
        for f in ("l", "r", "o", "z", "qk"):
            setattr(a, f, bufs[f].ptr)
        pi2 = (C.c_void_p * 1)(bufs["pi2"].ptr)
        a.pi2 = pi2
        for f in ("bl", "br", "bo", "bz", "alpha", "beta", "gamma"):
            setattr(a, f, host[f].ctypes.data)
        val, H = np.zeros(4, dtype=np.uint64), np.zeros(jac_words(cid, 0), dtype=np.uint64)
        keep += [d0, d1, pk, table, bufs, z_out, h_out, host, a, pi2, val, H]
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        calls["build_z"][curve] = lambda d0=d0, b=bufs, h=host, z=z_out: ctx.lib.check(ctx.lib.ga_plonk_build_z(
            d0.handle, b["l"].ptr, b["r"].ptr, b["o"].ptr, b["perm"].ptr, p(h["beta"]), p(h["gamma"]), 1, z.ptr))
        calls["quotient"][curve] = lambda pk=pk, a=a, o=h_out: ctx.lib.check(ctx.lib.ga_plonk_quotient_pinned(pk.handle, C.byref(a), o.ptr))
        calls["open"][curve] = lambda t=table, b=bufs, h=host, v=val, H=H: ctx.lib.check(ctx.lib.ga_kzg_open(
            t.handle, b["open"].ptr, n + 3, _lib.SCALARS_ON_DEVICE, p(h["point"]), p(v), p(H)))
        plans[curve] = {"srs_table_" + k: v for k, v in table.info().items()}
    res, total = {"plans": plans}, {NEW: [0.0] * reps, REF: [0.0] * reps}
    for name, cs in calls.items():
        ms = interleaved(ctx, reps, cs)
        res[name] = figure(ms)
        for k in total:
            total[k] = [x + y for x, y in zip(total[k], ms[k])]
    res["sum"] = figure(total)
    return res


RUNNERS = {"msm": run_msm, "fft": run_fft, "plonk": run_plonk}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", metavar="ITEM:LOGN", help="(child) measure one item")
    ap.add_argument("--items", nargs="+", default=["msm:20", "msm:22", "fft:22", "plonk:20"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per item")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bls12_377.json"))
    args = ap.parse_args()
    if args.one:
        import gnark_amd
        kind, logn = args.one.split(":")
        with gnark_amd.Context(0) as ctx:
            res = {"item": args.one, "log_n": int(logn), "reps": args.reps, "device": ctx.info()["name"].strip(), **RUNNERS[kind](ctx, int(logn), args.reps)}
        print(TAG + json.dumps(res), flush=True)
        return 0
    results = []
    for item in args.items:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--one", item, "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
        if r.returncode != 0 or not line:   # a failed step ends the run: nothing more is started on the device
            sys.stderr.write("step %s failed (exit %d)\n%s\n%s\n" % (item, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            return 1
        results.append(json.loads(line[0][len(TAG):]))
        print(line[0][:400], flush=True)
    findings = []
    for r in results:
        for k, v in r.items():
            if isinstance(v, dict) and "ratio" in v and not v["within_margin"]:
                findings.append({"item": r["item"], "figure": k, **v})
    doc = {"box": {"device": results[0]["device"] if results else None, "devices_used": 1},
           "method": "wall clock between ga_sync fences, median of `reps` repetitions after one warm-up per curve, the two curves interleaved in "
                     "one process on one context; operands in device memory; ratio = bls12-377 / bls12-381; bls12_381_spread = (max - min) / "
                     "median of the BLS12-381 repetitions of that run, the margin of `within_margin` (ratio <= 1 + spread)",
           "items": results, "expectation": "ratio <= 1 within the BLS12-381 spread: same limb counts and kernels, two scalar bits fewer",
           "findings": findings}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

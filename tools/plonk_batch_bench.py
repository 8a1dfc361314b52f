#!/usr/bin/env python3
"""Times the three batched PLONK calls -- ga_plonk_build_z_batch, ga_plonk_quotient_pinned_batch, ga_kzg_open_batch
(gnark_amd/csrc/plonk_batch.hip.h) -- against a loop over proofs of the three single calls on a library built from the PARENT commit,
and writes profiles/plonk_batch.json.

    the baseline is another checkout:
        git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/gnark_amd/csrc -j8 TARGET=$PWD/gnark_amd/variants/libgnark_amd_parent.so
    python tools/plonk_batch_bench.py [--parent-lib gnark_amd/variants/libgnark_amd_parent.so] [--log-n 10 12 14 16] [--counts 4 16]
                                      [--reps 10] [--out profiles/plonk_batch.json]

Every configuration (curve, size) runs in a child process of its own under `timeout`; the first child that fails ends the run.  Both
libraries are loaded into that one process, each with its own context, domains, pinned key (nb_bsb = 1) and SRS table of n + 3 points;
inputs and outputs live in device memory wherever the ABI allows it (the evaluation points, claimed values and H of an opening are
host arguments), and the timed runs are interleaved: batch, loop, batch, ...  A timed region starts and ends with ga_sync on its
context; the figure is the median wall-clock time of `reps` repetitions after one warm-up of each side, and the spread (max - min
over the median, per side) is recorded beside it: that spread is the margin of the condition below.  Per configuration and count the
file records
  * ms per proof of each of the three calls and of their sum, batch and baseline (the new build's own single path is not the baseline);
  * whether the outputs agree with the parent build's, per call (Z and h byte for byte; claimed values byte for byte and H after
    ga_jac_to_affine), and whether the claimed values equal Horner's rule in the C oracle -- an opening the two builds disagree on
    is decided by that;
  * one stage breakdown of the three batched calls from the stage profiler, taken in a separate pass.
The condition: at count 16 the median per-proof time of each batched call is no larger than the parent build's loop for that call,
within the recorded spread.  A configuration that misses it stays in the table and is reported as a finding.

--single times the SINGLE entry points of this build (ga_plonk_build_z, ga_plonk_quotient_pinned, ga_kzg_open: the one-proof case of
the batched drivers) against the parent build's single entry points, in the same way, and writes profiles/plonk_single_fold.json:
    python tools/plonk_batch_bench.py --single --configs bn254:10 bn254:16 bn254:22 bls12-381:16
The condition there: every call at every size and count is no slower than the parent's, within the recorded spread."""
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))

CURVES = ("bn254", "bls12-381")
CALLS = ("build_z", "quotient", "open")
TAG = "PLONK_BATCH_RESULT "
PROOF_FIELDS = ("l", "r", "o", "z", "qk")


def timed(ctx, call):
    ctx.sync()
    t0 = time.perf_counter()
    call()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3


def interleaved(reps, sides):
    """sides: [(ctx, call)]; one warm-up each, then reps rounds of every side in turn; per side (median, min, max) in ms"""
    for ctx, call in sides:
        timed(ctx, call)
    ms = [[] for _ in sides]
    for _ in range(reps):
        for k, (ctx, call) in enumerate(sides):
            ms[k].append(timed(ctx, call))
    return [(statistics.median(v), min(v), max(v)) for v in ms]


def older_library(path):
    """a build of an earlier commit through the current prototypes: entry points it does not have yet stay unbound"""
    from gnark_amd import _lib
    lib = _lib.Library.__new__(_lib.Library)
    lib.path, lib.dll = path, C.CDLL(path)
    for name, (res, args) in _lib._PROTOS.items():
        try:
            fn = getattr(lib.dll, name)
        except AttributeError:
            continue
        fn.restype, fn.argtypes = res, args
        setattr(lib, name, fn)
    return lib


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


class Side:
    """one library's view of the configuration: context, domains, pinned key, SRS table and the device copies of the inputs"""

    def __init__(self, ctx, curve, n, host, max_count):
        import numpy as np
        from gnark_amd import ecc, fft, plonk
        from gnark_amd.device import curve_id, jac_words
        self.ctx, self.lib, self.n, self.cid = ctx, ctx.lib, n, curve_id(curve)
        self.rho = plonk.Rho(n)
        self.d0, self.d1 = fft.Domain(ctx, curve, n), fft.Domain(ctx, curve, self.rho * n)
        self.pk = plonk.ProvingKey(self.d0, self.d1, host["fixed"], [host["qcp"]], lagrange=plonk.FIXED_IDS + ("Qcp0",))
        self.table = ecc.PrecomputedBases(ctx, curve, 0, host["srs"])
        self.jw = jac_words(self.cid, 0)
        self.bufs = {k: ctx.to_device(host[k]) for k in ("L", "R", "O", "Z", "Qk", "Pi2", "perm", "open")}
        self.z_out = ctx.malloc(max_count * n * 32)
        self.h_out = ctx.malloc(max_count * self.rho * n * 32)
        self.host, self.np = host, np
        self.vals, self.H = np.zeros((max_count, 4), dtype=np.uint64), np.zeros((max_count, self.jw), dtype=np.uint64)

    def struct(self, ins, j):
        from gnark_amd import _lib
        a, n, h = ins[j], self.n, self.host
        a.nb_bsb, a.flags = 1, 1   # GA_PLONK_ON_DEVICE
        a.lagrange_mask = sum(1 << k for k in (0, 1, 2, 3, 8, 13))   # L R O Z Qk Pi2_0 as evaluations (s.x before computeNumerator)
        for f, k in zip(PROOF_FIELDS, ("L", "R", "O", "Z", "Qk")):
            setattr(a, f, self.bufs[k].offset(j * n * 32))
        self.keep.append((C.c_void_p * 1)(self.bufs["Pi2"].offset(j * n * 32)))
        a.pi2 = self.keep[-1]
        for f in ("bl", "br", "bo", "bz"):
            setattr(a, f, h[f][j].ctypes.data)
        for f, k in (("alpha", "alpha"), ("beta", "betas"), ("gamma", "gammas")):
            setattr(a, f, h[k][j:j + 1].ctypes.data)

    def prepare(self, count):
        from gnark_amd import _lib
        self.keep = []
        self.ins = (_lib.PlonkQuotientIn * count)()
        for j in range(count):
            self.struct(self.ins, j)
        m = self.host["open"].shape[1]
        self.polys = (C.c_void_p * count)(*[self.bufs["open"].offset(j * m * 32) for j in range(count)])

    # the batched calls (new build) and the loops of single calls (parent build), all on device buffers
    def batch(self, call, count):
        from gnark_amd import _lib
        lib, h, b, n = self.lib, self.host, self.bufs, self.n
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        if call == "build_z":
            lib.check(lib.ga_plonk_build_z_batch(self.d0.handle, b["L"].ptr, b["R"].ptr, b["O"].ptr, b["perm"].ptr, p(h["betas"]), p(h["gammas"]),
                                                 count, 1, self.z_out.ptr))
        elif call == "quotient":
            lib.check(lib.ga_plonk_quotient_pinned_batch(self.pk.handle, self.ins, count, self.h_out.ptr))
        else:
            lib.check(lib.ga_kzg_open_batch(self.table.handle, self.polys, h["open"].shape[1], count, _lib.SCALARS_ON_DEVICE, p(h["points"]), p(self.vals), p(self.H)))

    def loop(self, call, count):
        from gnark_amd import _lib
        lib, h, b, n = self.lib, self.host, self.bufs, self.n
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        for j in range(count):
            if call == "build_z":
                lib.check(lib.ga_plonk_build_z(self.d0.handle, b["L"].offset(j * n * 32), b["R"].offset(j * n * 32), b["O"].offset(j * n * 32),
                                               b["perm"].ptr, p(h["betas"][j:j + 1]), p(h["gammas"][j:j + 1]), 1, self.z_out.offset(j * n * 32)))
            elif call == "quotient":
                lib.check(lib.ga_plonk_quotient_pinned(self.pk.handle, C.byref(self.ins[j]), self.h_out.offset(j * self.rho * n * 32)))
            else:
                lib.check(lib.ga_kzg_open(self.table.handle, self.polys[j], h["open"].shape[1], _lib.SCALARS_ON_DEVICE, p(h["points"][j:j + 1]), p(self.vals[j:j + 1]),
                                          p(self.H[j:j + 1])))

    def outputs(self, count):
        np = self.np
        aff = np.zeros((count, 2 * self.jw // 3), dtype=np.uint64)
        for j in range(count):
            self.lib.check(self.lib.ga_jac_to_affine(self.cid, 0, self.H[j].ctypes.data, aff[j].ctypes.data))
        return [self.z_out.to_host((count, self.n, 4)), self.h_out.to_host((count, self.rho * self.n, 4)), self.vals[:count].copy(), aff]

    def close(self):
        for b in list(self.bufs.values()) + [self.z_out, self.h_out]:
            b.free()
        self.table.free()
        self.pk.close()
        self.d0.close()
        self.d1.close()


def run_config(curve, logn, counts, reps, parent_lib, single=False):
    import numpy as np
    import gnark_amd
    import oracle
    from gnark_amd import plonk, synth
    from gnark_amd.device import curve_id
    new, par = gnark_amd.Context(0), gnark_amd.Context(0, lib=older_library(parent_lib))
    cid, n, mc = curve_id(curve), 1 << logn, max(counts)
    gen = lambda count, seed: synth._gen_scalars(new, cid, count, seed)
    host = {k: gen(mc * n, 0x910 + i).reshape(mc, n, 4) for i, k in enumerate(("L", "R", "O", "Z", "Qk", "Pi2"))}
    host["fixed"] = {k: gen(n, 0x920 + i) for i, k in enumerate(plonk.FIXED_IDS)}
    host["qcp"] = gen(n, 0x930)
    host["perm"] = np.random.default_rng(0x940 + logn).permutation(3 * n).astype(np.int64)
    host["open"] = gen(mc * (n + 3), 0x950).reshape(mc, n + 3, 4)   # blinded polynomials: n + 3 coefficients
    host["srs"] = synth._gen_bases(new, cid, 0, n + 3, 0x960, False)[0]
    for i, (k, cnt) in enumerate((("bl", 2), ("br", 2), ("bo", 2), ("bz", 3))):
        host[k] = gen(mc * cnt, 0x970 + i).reshape(mc, cnt, 4)
    for i, k in enumerate(("alpha", "betas", "gammas", "points")):
        host[k] = gen(mc, 0x980 + i)
    sides = [Side(new, curve, n, host, mc), Side(par, curve, n, host, mc)]
    rows = []
    try:
        for count in counts:
            for s in sides:
                s.prepare(count)
            run_new = sides[0].loop if single else sides[0].batch   # what is measured against the parent build's loop
            for call in CALLS:
                run_new(call, count)
                sides[1].loop(call, count)
            got, ref = sides[0].outputs(count), sides[1].outputs(count)
            eq = [bool(np.array_equal(a, b)) for a, b in zip(got, ref)]
            horner = [[bool(np.array_equal(v[j], oracle.fr_horner(cid, host["open"][j], host["points"][j]))) for j in range(count)] for v in (got[2], ref[2])]
            row = {"count": count, "outputs_equal": {"build_z": eq[0], "quotient": eq[1], "open": eq[2] and eq[3]},
                   "claimed_values_equal_horner": {"batch": all(horner[0]), "parent_loop": all(horner[1])}}
            tot = {"batch": 0.0, "parent": 0.0}
            for call in CALLS:
                (b, bmin, bmax), (l, lmin, lmax) = interleaved(reps, [(new, lambda: run_new(call, count)),
                                                                       (par, lambda: sides[1].loop(call, count))])
                spread = max((bmax - bmin) / b, (lmax - lmin) / l)
                row[call] = {"batch_ms_per_proof": round(b / count, 4), "parent_loop_ms_per_proof": round(l / count, 4),
                             "batch_min_ms_per_proof": round(bmin / count, 4), "parent_loop_min_ms_per_proof": round(lmin / count, 4),
                             "parent_over_batch": round(l / b, 3), "spread": round(spread, 3), "no_slower": bool(b <= l * (1 + spread))}
                tot["batch"] += b
                tot["parent"] += l
            row["sum"] = {"batch_ms_per_proof": round(tot["batch"] / count, 4), "parent_loop_ms_per_proof": round(tot["parent"] / count, 4),
                          "parent_over_batch": round(tot["parent"] / tot["batch"], 3)}
            row["batch_stages_ms"] = stage_profile(new, lambda: [run_new(call, count) for call in CALLS])
            rows.append(row)
    finally:
        for s in sides:
            s.close()
    res = {"curve": curve, "log_n": logn, "nb_bsb": 1, "reps": reps, "batch_side": "loop of single calls" if single else "batched calls", "device": new.info()["name"].strip(), "counts": rows}
    new.close()
    par.close()
    print(TAG + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=2, metavar=("CURVE", "LOGN"), help="(child) measure one configuration")
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "gnark_amd", "variants", "libgnark_amd_parent.so"))
    ap.add_argument("--log-n", type=int, nargs="+", default=[10, 12, 14, 16])
    ap.add_argument("--counts", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--curves", nargs="+", default=list(CURVES))
    ap.add_argument("--configs", nargs="+", metavar="CURVE:LOGN", help="these configurations instead of every --curves x --log-n")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per configuration")
    ap.add_argument("--single", action="store_true", help="time this build's single entry points (the `batch` columns then hold them)")
    ap.add_argument("--out", default=None, help="default: profiles/plonk_batch.json, or profiles/plonk_single_fold.json with --single")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "plonk_single_fold.json" if args.single else "plonk_batch.json")
    if args.single and args.counts == [4, 16]:
        args.counts = [1]
    if not os.path.exists(args.parent_lib):
        sys.stderr.write("%s not found: build the parent commit's library first (see the top of this file)\n" % args.parent_lib)
        return 2
    if args.one:
        run_config(args.one[0], int(args.one[1]), args.counts, args.reps, args.parent_lib, args.single)
        return 0
    results = []
    configs = [(curve, logn) for logn in args.log_n for curve in args.curves]
    if args.configs:
        configs = [(c.rsplit(":", 1)[0], int(c.rsplit(":", 1)[1])) for c in args.configs]
    for curve, logn in configs:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--one", curve, str(logn),
               "--parent-lib", args.parent_lib, "--reps", str(args.reps)] + (["--single"] if args.single else [])
        r = subprocess.run(cmd + ["--counts"] + [str(k) for k in args.counts], capture_output=True, text=True, cwd=ROOT)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
        if r.returncode != 0 or not line:   # a failed step ends the run: nothing more is started on the device
            sys.stderr.write("step %s failed (exit %d)\n%s\n%s\n" % ((curve, logn), r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            return 1
        results.append(json.loads(line[0][len(TAG):]))
        print(line[0][:300], flush=True)
    cond = {"what": "count = 16, n <= 2^16, both curves: the median per-proof time of each batched call is no larger than the parent build's "
                    "loop of the single call, within the recorded run-to-run spread", "missed": []}
    if args.single:
        cond["what"] = ("every size and count, both curves: the median time of each single call of this build is no larger than the parent "
                        "build's single call, within the recorded run-to-run spread")
    for r in results:
        for row in r["counts"]:
            if args.single or row["count"] == 16:
                for call in CALLS:
                    if not row[call]["no_slower"]:
                        cond["missed"].append({"curve": r["curve"], "log_n": r["log_n"], "call": call, **row[call]})
    cond["met"] = not cond["missed"]
    doc = {"box": {"device": results[0]["device"] if results else None, "devices_used": 1},
           "method": "wall clock between ga_sync fences, median of `reps` interleaved repetitions after one warm-up of each side; the baseline "
                     "is a loop over proofs of the single call on a library built from the parent commit, loaded into the same process; one "
                     "pinned key with nb_bsb = 1, an SRS table of n + 3 points, polynomials of n + 3 coefficients opened; inputs and outputs "
                     "in device memory (evaluation points, claimed values and H are host arguments of the ABI); spread = (max - min) / median",
           "configurations": results, "condition": cond}
    if args.single:
        doc["method"] = doc["method"].replace("the baseline is a loop", "the `batch` columns are a loop over proofs of this build's SINGLE call; the baseline is a loop")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

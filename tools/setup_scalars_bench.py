#!/usr/bin/env python3
"""Times the Fr vector calls of groth16.Setup's scalar side -- ga_fr_sparse_matvec (gnark_amd/csrc/fr_sparse.hip.h), ga_fr_lagrange_at
and ga_fr_compact_nonzero (fr_setup.hip.h) -- and writes profiles/setup_scalars.json.

    python tools/setup_scalars_bench.py [--log-rows 20] [--log-long 20] [--log-n 20] [--reps 5]

One process, both curves.  x and the output are on the device; `kernels_ms` is the sum of the stage profiler's hipEvents, `wall_ms` the
whole call with the profiler off: the host's validation walk over the matrix, the segment list and the upload of terms and segments
included.  Recorded, nothing gated:
  matvec    two matrices over 2^16 x values and 256 coefficients: 2^log-rows rows x 3 terms, and the same with one row of 2^log-long
            terms in the middle (the constant wire).  Bytes moved = 40 B per term (8 B of term, 32 B of gathered x), 12 B per segment,
            32 B per partial sum written and read again, 32 B per row; bytes/s over the kernels, beside a device-to-device hipMemcpy (the
            same process) that moves the same number of bytes (half of them read, half written).
  segment   the skewed matrix for GA_FR_SPARSE_SEGMENT in {8, 16, 32, 64}: kernels and whole call.
  lagrange, compact   ga_fr_lagrange_at and ga_fr_compact_nonzero (30 % zeros, device to device) at 2^log-n.
There is no CPU figure: gnark is not available to this repository, and none is made up."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

CURVES = ("bn254", "bls12-381")
SEGMENTS = (8, 16, 32, 64)
N_COEFFS = 256
DEFAULT_SEGMENT = 32   # FR_SPARSE_DEFAULT_SEGMENT of fr_sparse.hip.h: the segment length of the `matvec` records (their byte count follows it)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, default=20)
    ap.add_argument("--log-cols", type=int, default=16)
    ap.add_argument("--log-long", type=int, default=20)
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another build of the library (the functional emulation, at small sizes; no copy yardstick then)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "setup_scalars.json"))
    args = ap.parse_args()

    import gnark_amd
    import pyref
    from gnark_amd import _lib
    from gnark_amd.device import Context, curve_id

    class Hip:
        """hipMemcpyAsync and hipEvents of the HIP runtime the library itself has loaded (found in this process's maps)"""

        def __init__(self):
            paths = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
            if len(paths) != 1:   # two runtimes in one process: the buffers of one are no pointers for the other
                raise RuntimeError("expected exactly one HIP runtime in the process, found %r" % paths)
            self.dll = C.CDLL(paths[0])
            for name in ("hipEventCreate", "hipEventRecord", "hipEventSynchronize", "hipEventElapsedTime", "hipMemcpyAsync", "hipEventDestroy"):
                getattr(self.dll, name).restype = C.c_int

        def check(self, rc, what):
            if rc != 0:
                raise RuntimeError("%s failed: hipError %d" % (what, rc))

        def copy_ms(self, dst, src, nbytes):
            a, b, ms = C.c_void_p(), C.c_void_p(), C.c_float()
            self.check(self.dll.hipEventCreate(C.byref(a)), "hipEventCreate")
            self.check(self.dll.hipEventCreate(C.byref(b)), "hipEventCreate")
            self.check(self.dll.hipEventRecord(a, None), "hipEventRecord")
            self.check(self.dll.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(nbytes), 3, None), "hipMemcpyAsync")   # 3 = hipMemcpyDeviceToDevice
            self.check(self.dll.hipEventRecord(b, None), "hipEventRecord")
            self.check(self.dll.hipEventSynchronize(b), "hipEventSynchronize")
            self.check(self.dll.hipEventElapsedTime(C.byref(ms), a, b), "hipEventElapsedTime")
            self.dll.hipEventDestroy(a)
            self.dll.hipEventDestroy(b)
            return ms.value

    def copy_rate(ctx, nbytes):
        """bytes moved per second by a device-to-device hipMemcpy of nbytes / 2 (read + written = nbytes): a warm-up, then the best of reps"""
        if args.lib:
            return None
        hip = Hip()
        src, dst = ctx.malloc(nbytes // 2), ctx.malloc(nbytes // 2)
        try:
            hip.copy_ms(dst.ptr, src.ptr, nbytes // 2)
            best = min(hip.copy_ms(dst.ptr, src.ptr, nbytes // 2) for _ in range(args.reps))
        finally:
            src.free()
            dst.free()
        return {"copy_ms": round(best, 3), "bytes_per_s": round(nbytes / (best * 1e-3))}

    doc = {"matvec": [], "segment": [], "lagrange": [], "compact": []}
    ctx = Context(0, lib=_lib.Library(args.lib)) if args.lib else gnark_amd.Context(0)
    with ctx:
        lib, h = ctx.lib, ctx.handle
        dev = _lib.VECTOR_ON_DEVICE | _lib.RESULT_ON_DEVICE | _lib.SCALARS_MONTGOMERY

        def profiled(call):
            ctx.profile(True)
            ctx.profile_reset()
            call()
            st = {}
            for name, ms in ctx.profile_read():
                st[name] = st.get(name, 0.0) + ms
            ctx.profile(False)
            return st

        def best(call, env=None):
            """under `env`: a warm-up, `reps` profiled calls (the stage ms of the fastest by kernel time), then `reps` calls with the
            profiler off (the fastest whole call, host clock: every entry point returns after its stream is idle)"""
            for k, v in (env or {}).items():
                os.environ[k] = str(v)
            try:
                call()
                runs = [profiled(call) for _ in range(args.reps)]
                walls = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    call()
                    walls.append((time.perf_counter() - t0) * 1e3)
            finally:
                for k in (env or {}):
                    os.environ.pop(k, None)
            st = min(runs, key=lambda x: sum(x.values()))
            return {k: round(v, 3) for k, v in st.items()}, round(min(walls), 3)

        for curve in CURVES:
            cid = curve_id(curve)
            c = pyref.BN254 if cid == 0 else pyref.BLS12_381
            rng = np.random.default_rng(0x5E7B + cid)

            def rand_words(m):   # values below r (read as fr.Element images)
                w = rng.integers(0, 1 << 64, size=(m, 4), dtype=np.uint64)
                w[:, 3] = rng.integers(1, c.r >> 192, size=m, dtype=np.uint64)
                return w
            n_rows, n_cols = 1 << args.log_rows, 1 << args.log_cols
            d_x, coeffs = ctx.to_device(rand_words(n_cols)), rand_words(N_COEFFS)
            d_out = ctx.malloc((n_rows + 1) * 32)

            def matvec_call(row_start, terms):
                def call():
                    lib.check(lib.ga_fr_sparse_matvec(h, cid, C.c_void_p(d_x.ptr), n_cols, row_start.ctypes.data_as(C.c_void_p), row_start.size - 1,
                                                      terms.ctypes.data_as(C.c_void_p), coeffs.ctypes.data_as(C.c_void_p), N_COEFFS, None, None, 0, dev,
                                                      C.c_void_p(d_out.ptr)))
                return call

            def traffic(row_start, S):
                """bytes the kernels move, from the shape of the segments"""
                lengths = np.diff(row_start.astype(np.int64))
                total = int(row_start[-1]) * 40 + lengths.size * 32
                while True:
                    segs = (np.maximum(lengths, 1) + S - 1) // S
                    total += int(segs.sum()) * 12
                    lengths = segs[segs > 1]
                    if lengths.size == 0:
                        return total
                    total += int(lengths.sum()) * 64   # partial sums: written by one level, read by the next

            terms = np.empty((3 * n_rows, 2), np.uint32)
            terms[:, 0] = rng.integers(0, N_COEFFS, size=3 * n_rows)
            terms[:, 1] = rng.integers(0, n_cols, size=3 * n_rows)
            uniform = (np.arange(n_rows + 1, dtype=np.uint64) * 3, terms)
            long_terms = np.empty((1 << args.log_long, 2), np.uint32)
            long_terms[:, 0] = rng.integers(0, N_COEFFS, size=long_terms.shape[0])
            long_terms[:, 1] = rng.integers(0, n_cols, size=long_terms.shape[0])
            half = n_rows // 2
            skew_start = np.concatenate([uniform[0][:half + 1], uniform[0][half:] + np.uint64(long_terms.shape[0])])
            skewed = (skew_start, np.concatenate([terms[:3 * half], long_terms, terms[3 * half:]]))
            assert skew_start.size == n_rows + 2 and skew_start[-1] == skewed[1].shape[0] and (np.diff(skew_start.astype(np.int64)) >= 0).all()
            for name, (row_start, tm) in (("uniform", uniform), ("skewed", skewed)):
                st, wall = best(matvec_call(row_start, tm))
                nbytes = traffic(row_start, DEFAULT_SEGMENT)
                kernels = sum(st.values())
                rec = {"curve": curve, "matrix": name, "rows": row_start.size - 1, "terms": int(row_start[-1]), "stages_ms": st, "kernels_ms": round(kernels, 3),
                       "wall_ms": wall, "bytes_moved": nbytes, "bytes_per_s": round(nbytes / (kernels * 1e-3)), "device_copy_same_bytes": copy_rate(ctx, nbytes)}
                doc["matvec"].append(rec)
                print("SETUP_MATVEC " + json.dumps(rec), flush=True)
            table = {}
            for S in SEGMENTS:
                st, wall = best(matvec_call(*skewed), {"GA_FR_SPARSE_SEGMENT": S})
                table[str(S)] = {"levels": len(st), "kernels_ms": round(sum(st.values()), 3), "level_ms": [st[k] for k in sorted(st)], "wall_ms": wall}
            rec = {"curve": curve, "rows": skew_start.size - 1, "long_row_terms": long_terms.shape[0], "segment": table}
            doc["segment"].append(rec)
            print("SETUP_SEGMENT " + json.dumps(rec), flush=True)
            d_x.free()
            d_out.free()

            n = 1 << args.log_n
            tau = rand_words(1)
            d_lag = ctx.malloc(n * 32)
            st, wall = best(lambda: lib.check(lib.ga_fr_lagrange_at(h, cid, n, tau.ctypes.data_as(C.c_void_p), n, dev, C.c_void_p(d_lag.ptr))))
            rec = {"curve": curve, "log_n": args.log_n, "stages_ms": st, "kernels_ms": round(sum(st.values()), 3), "wall_ms": wall}
            doc["lagrange"].append(rec)
            print("SETUP_LAGRANGE " + json.dumps(rec), flush=True)
            v = rand_words(n)
            v[rng.integers(0, 10, size=n) < 3] = 0
            d_v = ctx.to_device(v)
            count = C.c_uint64(0)
            mask = np.zeros(n, np.uint8)
            st, wall = best(lambda: lib.check(lib.ga_fr_compact_nonzero(h, cid, C.c_void_p(d_v.ptr), n, dev, C.c_void_p(d_lag.ptr), mask.ctypes.data_as(C.c_void_p),
                                                                        C.byref(count))))
            rec = {"curve": curve, "log_n": args.log_n, "kept": count.value, "stages_ms": st, "kernels_ms": round(sum(st.values()), 3), "wall_ms": wall}
            doc["compact"].append(rec)
            print("SETUP_COMPACT " + json.dumps(rec), flush=True)
            d_lag.free()
            d_v.free()
    doc["cpu_reference"] = None
    doc["cpu_reference_note"] = "gnark's groth16.Setup was not available where this was measured: no CPU figure"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

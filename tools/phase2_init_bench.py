#!/usr/bin/env python3
"""Times the two device calls of Groth16 Phase2.Initialize -- ga_sparse_point_sums (gnark_amd/csrc/sparse_sums.hip.h) and
ga_lagrange_coeffs (ec_ntt.hip.h) -- and writes profiles/phase2_init.json.

    python tools/phase2_init_bench.py [--log-rows 20] [--g2-log-rows 18] [--log-long 20] [--lagrange-log-n 12 16 18] [--reps 3]

One process.  Points and output are on the device; kernel times are the hipEvents of the stage profiler, `wall_ms` is the whole call
(the host's walk over the matrix and the upload of its codes included).  Recorded, nothing gated:
  sparse    2^log-rows rows x 3 terms over 2^16 points, G1 of both curves (G2 at 2^g2-log-rows), for three coefficient mixes: all +-1,
            10 % general full-width, all general (256 distinct general coefficients, as a circuit has few).  Per mix: ms per stage,
            point operations/s (the products' doublings and additions counted from the digits of the magnitudes, as
            tools/scale_points_bench.py counts them, plus one addition per term beyond a row's first), and beside them, in the same
            process, ga_scale_points on as many points as there are general terms with the same scalars (the product stage is that
            ladder plus a gather: the ratio is what the gather costs) and the fixed-base accumulation kernel's rate, the yardstick
            profiles/to_lagrange.json uses for additions.
  segment   one row of 2^log-long terms among 2^16 rows of 3, all +-1: the row-sum stages for GA_SPARSE_SEGMENT in {8, 16, 32, 64, 128}.
  order     the products of the two general mixes with GA_SPARSE_ORDER=0 (row order) and 1 (sorted by coefficient id).
  lagrange  ga_lagrange_coeffs on G2 beside G1 at the same sizes; the expectation to compare with is the G2 / G1 ratio per
            multiplication of the plain ladder in profiles/scale_points.json.
There is no CPU figure: gnark-crypto is not available to this repository, and none is made up."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

CURVES = ("bn254", "bls12-381")
MIXES = {"pm1": 0.0, "general10": 0.10, "general": 1.0}
SEGMENTS = (8, 16, 32, 64, 128)
N_GENERAL = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, default=20)
    ap.add_argument("--g2-log-rows", type=int, default=18)
    ap.add_argument("--log-points", type=int, default=16)
    ap.add_argument("--log-long", type=int, default=20)
    ap.add_argument("--lagrange-log-n", type=int, nargs="*", default=[12, 16, 18])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lib", default=None, help="another build of the library (the functional emulation, at small sizes)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phase2_init.json"))
    args = ap.parse_args()

    import gnark_amd
    import pyref
    from gnark_amd import _lib, ecc
    from gnark_amd.device import Context, affine_words, curve_id
    from helpers import gen_of, pts_to_arr
    from scale_points_bench import op_counts, to_words

    doc = {"sparse": [], "segment": [], "order": [], "lagrange": [], "yardstick": []}
    ctx = Context(0, lib=_lib.Library(args.lib)) if args.lib else gnark_amd.Context(0)
    with ctx:
        lib = ctx.lib

        def profiled(call):
            ctx.profile(True)
            ctx.profile_reset()
            t0 = time.perf_counter()
            ret = call()
            wall = (time.perf_counter() - t0) * 1e3
            st = {}
            for name, ms in ctx.profile_read():
                st[name] = st.get(name, 0.0) + ms
            ctx.profile(False)
            return st, wall, ret

        def best(call, env=None):
            """a warm-up, then `reps` profiled calls under `env`: (stage ms of the fastest call by kernel time, its wall ms, redone)"""
            for k, v in (env or {}).items():
                os.environ[k] = str(v)
            try:
                call()
                runs = [profiled(call) for _ in range(args.reps)]
            finally:
                for k in (env or {}):
                    os.environ.pop(k, None)
            st, wall, red = min(runs, key=lambda x: sum(x[0].values()))
            return {k: round(v, 3) for k, v in st.items()}, round(min(w for _, w, _ in runs), 3), red

        for curve in CURVES:
            cid = curve_id(curve)
            c = pyref.BN254 if cid == 0 else pyref.BLS12_381
            rtop = c.r >> 192
            for group, log_rows in ((0, args.log_rows), (1, args.g2_log_rows)):
                rng = np.random.default_rng(0xF2A5E + 1000 * cid + group)
                wa, n_rows, n_points = affine_words(cid, group), 1 << log_rows, 1 << args.log_points

                def rand_words(m):   # full-width scalars below r: the top word below r's
                    w = rng.integers(0, 1 << 64, size=(m, 4), dtype=np.uint64)
                    w[:, 3] = rng.integers(1, rtop, size=m, dtype=np.uint64)
                    return w
                base = pts_to_arr(c, group, [gen_of(c, group)])
                nmax = max(n_points, 3 * n_rows)
                logs, pts = ctx.to_device(rand_words(nmax)), ctx.malloc(nmax * wa * 8)

                def make_points():   # nmax random multiples of the generator: the points, and the input of the ga_scale_points runs
                    lib.check(lib.ga_batch_scalar_mul(ctx.handle, cid, group, base.ctypes.data_as(C.c_void_p), C.c_void_p(logs.ptr), nmax,
                                                      _lib.SCALARS_ON_DEVICE | _lib.RESULT_ON_DEVICE, C.c_void_p(pts.ptr)))
                make_points()
                fb, _, _ = profiled(make_points)
                nwin = ecc.batch_scalar_mul_plan(curve, nmax, lib=lib)[1]
                yard_rate = nwin * nmax / (fb["fixed_base_accumulate"] * 1e-3)
                doc["yardstick"].append({"curve": curve, "group": "G2" if group else "G1", "n": nmax, "fixed_base_accumulate_ms": round(fb["fixed_base_accumulate"], 3),
                                         "windows": nwin, "additions_per_s": round(yard_rate)})
                # coefficients: +1, -1, then N_GENERAL full-width values; their magnitudes min(c, r - c) are what the ladder sees
                gen_words = rand_words(N_GENERAL)
                gen_ints = [int.from_bytes(row.tobytes(), "little") for row in gen_words]
                coeffs = np.concatenate([to_words([1, c.r - 1]), gen_words])
                mags = to_words([min(k, c.r - k) for k in gen_ints])
                out = ctx.malloc(max(n_rows, (1 << 16) + 1) * wa * 8)
                scaled = ctx.malloc(3 * n_rows * wa * 8)

                def sparse_call(row_start, terms):
                    red = C.c_uint64(0)

                    def call():
                        lib.check(lib.ga_sparse_point_sums(ctx.handle, cid, group, C.c_void_p(pts.ptr), n_points, row_start.ctypes.data_as(C.c_void_p),
                                                           row_start.size - 1, terms.ctypes.data_as(C.c_void_p), coeffs.ctypes.data_as(C.c_void_p), coeffs.shape[0],
                                                           _lib.BASES_ON_DEVICE | _lib.RESULT_ON_DEVICE, C.c_void_p(out.ptr), C.byref(red)))
                        return red.value
                    return call

                def matrix(rows, per_row, frac):
                    nnz = rows * per_row
                    terms = np.empty((nnz, 2), np.uint32)
                    terms[:, 0] = rng.integers(0, 2, size=nnz)
                    general = rng.random(nnz) < frac
                    terms[general, 0] = 2 + rng.integers(0, N_GENERAL, size=int(general.sum()))
                    # distinct columns inside a row: a random start and odd steps
                    start = rng.integers(0, n_points, size=rows)
                    terms[:, 1] = ((start[:, None] + np.arange(per_row)[None, :] * (1 + 2 * rng.integers(0, 64, size=rows))[:, None]) % n_points).reshape(-1)
                    return np.arange(rows + 1, dtype=np.uint64) * per_row, terms, general

                for mix, frac in MIXES.items():
                    row_start, terms, general = matrix(n_rows, 3, frac)
                    ngen = int(general.sum())
                    st, wall, red = best(sparse_call(row_start, terms))
                    rec = {"curve": curve, "group": "G2" if group else "G1", "log_rows": log_rows, "terms_per_row": 3, "mix": mix, "general_terms": ngen,
                           "stages_ms": st, "kernels_ms": round(sum(st.values()), 3), "wall_ms": wall, "redone": red}
                    ops = 2 * n_rows   # one addition per term beyond the first of a row
                    if ngen:
                        w = mags[terms[general, 0] - 2]
                        o = op_counts(w)["window"]
                        ops += o["lane_doublings"] + o["lane_additions"]
                        d_s = ctx.to_device(w)
                        red2 = C.c_uint64(0)

                        def scale():
                            lib.check(lib.ga_scale_points(ctx.handle, cid, group, C.c_void_p(pts.ptr), ngen, _lib.SCALE_EACH, C.c_void_p(d_s.ptr), 0,
                                                          _lib.SCALARS_ON_DEVICE | _lib.BASES_ON_DEVICE | _lib.RESULT_ON_DEVICE, C.c_void_p(scaled.ptr), C.byref(red2)))
                        sst, _, _ = best(scale)
                        d_s.free()
                        rec["scale_points_same_terms_ladder_ms"] = sst["scale_ladder"]
                        rec["products_over_scale_points_ladder"] = round(st["sparse_products"] / sst["scale_ladder"], 4)
                    rec["point_ops"] = int(ops)
                    rec["point_ops_per_s"] = round(ops / (sum(st.values()) * 1e-3))
                    rec["point_ops_per_s_over_yardstick"] = round(rec["point_ops_per_s"] / yard_rate, 4)
                    doc["sparse"].append(rec)
                    print("PHASE2_SPARSE " + json.dumps(rec), flush=True)
                    if ngen and group == 0:
                        orders = {}
                        for order in (0, 1):
                            ost, owall, _ = best(sparse_call(row_start, terms), {"GA_SPARSE_ORDER": order})
                            orders["cid" if order else "row"] = {"products_ms": ost["sparse_products"], "kernels_ms": round(sum(ost.values()), 3), "wall_ms": owall}
                        rec = {"curve": curve, "log_rows": log_rows, "mix": mix, **orders,
                               "cid_over_row_products": round(orders["cid"]["products_ms"] / orders["row"]["products_ms"], 4)}
                        doc["order"].append(rec)
                        print("PHASE2_ORDER " + json.dumps(rec), flush=True)
                if group == 0:
                    # one long row (the constant wire) in the middle of short ones
                    short = 1 << 16
                    rs, tm, _ = matrix(short, 3, 0.0)
                    long_terms = np.empty((1 << args.log_long, 2), np.uint32)
                    long_terms[:, 0] = rng.integers(0, 2, size=long_terms.shape[0])
                    long_terms[:, 1] = rng.integers(0, n_points, size=long_terms.shape[0])
                    half = 3 * (short // 2)
                    terms = np.concatenate([tm[:half], long_terms, tm[half:]])
                    row_start = np.concatenate([rs[:short // 2 + 1], rs[short // 2 + 1:] + np.uint64(long_terms.shape[0])])
                    row_start = np.insert(row_start, short // 2 + 1, rs[short // 2] + np.uint64(long_terms.shape[0]))
                    assert row_start.size == short + 2 and row_start[-1] == terms.shape[0] and (np.diff(row_start.astype(np.int64)) >= 0).all()
                    table = {}
                    for S in SEGMENTS:
                        st, wall, red = best(sparse_call(row_start, terms), {"GA_SPARSE_SEGMENT": S})
                        sums = {k: v for k, v in st.items() if k.startswith("sparse_sums")}
                        table[str(S)] = {"levels": len(sums), "sums_ms": round(sum(sums.values()), 3), "level_ms": [sums[k] for k in sorted(sums)], "wall_ms": wall,
                                         "redone": red}
                    rec = {"curve": curve, "short_rows": short, "long_row_terms": long_terms.shape[0], "segment": table}
                    doc["segment"].append(rec)
                    print("PHASE2_SEGMENT " + json.dumps(rec), flush=True)
                for b in (logs, pts, out, scaled):
                    b.free()
            # the transform: G2 beside G1, the same sizes, the same process
            for logn in args.lagrange_log_n:
                n, rec = 1 << logn, {"curve": curve, "log_n": logn}
                for group in (0, 1):
                    wa = affine_words(cid, group)
                    rng = np.random.default_rng(0x1A6 + logn + group)
                    w = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
                    w[:, 3] = rng.integers(1, rtop, size=n, dtype=np.uint64)
                    d_in = ecc.BatchScalarMultiplication(ctx, curve, group, pts_to_arr(c, group, [gen_of(c, group)]), w, out_device=True)
                    d_out = ctx.malloc(n * wa * 8)

                    def call():
                        lib.check(lib.ga_lagrange_coeffs(ctx.handle, cid, group, C.c_void_p(d_in.ptr), n, _lib.BASES_ON_DEVICE | _lib.RESULT_ON_DEVICE,
                                                         C.c_void_p(d_out.ptr)))
                    st, wall, _ = best(call)
                    stages = sum(v for k, v in st.items() if k.startswith("ec_ntt_stage"))
                    rec["G2" if group else "G1"] = {"kernels_ms": round(sum(st.values()), 3), "stages_ms": round(stages, 3), "wall_ms": wall,
                                                    "multiplications_per_s": round((n // 2) * logn / (stages * 1e-3)) if stages else None}
                    d_in.free()
                    d_out.free()
                rec["g2_over_g1"] = round(rec["G2"]["kernels_ms"] / rec["G1"]["kernels_ms"], 3)
                doc["lagrange"].append(rec)
                print("PHASE2_LAGRANGE " + json.dumps(rec), flush=True)
    doc["cpu_reference"] = None
    doc["cpu_reference_note"] = "gnark's mpcsetup was not available where this was measured: no CPU figure"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Times ga_pairing_check (gnark_amd/csrc/pairing.hip.h) and the verifiers of gnark_amd/g16_verify.py on the device and writes
profiles/pairing.json.

    python tools/pairing_bench.py [--log-n 10 12 14 16] [--reps 3] [--curves bn254 bls12-381] [--proofs-log-n 12] [--out profiles/pairing.json]

One process.  Per curve and size: one group of 2^log-n pairs ([a_i]G1, [b_i]G2), points on the device, no output but out2; the three
stage times are the hipEvents of the stage profiler, the call's milliseconds their sum, once warm and then `reps` times.  The Miller
kernel's rate in Fp2 products per second uses the products per pair counted from the formulas (products_per_pair below),
and is set beside the rate of the G2 ladder of ga_scale_points (GA_SCALE_WINDOW=0, full-width scalars: 9 products a doubling, 14 an
addition) on the same Q in the same process: both are one-lane-per-item Fp2 arithmetic, the ladder on the lazy 29-bit layer and the
Miller loop on the exact one -- the ratio is the datum for moving the loop onto the lazy layer.  Then VerifyMany and BatchVerify on
2^proofs-log-n proofs of a key with one public input (the cubic circuit's size), wall clock with the host work included.  The
proofs are made to satisfy the verification equation from known logarithms (Krs = [(xy - ab - k g)/d]G1): what a prover would send.
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

import numpy as np  # noqa: E402

CURVES = ("bn254", "bls12-381")
LOOP = {"bn254": 6 * 4965661367192848881 + 2, "bls12-381": 0xd201000000010000}
# Fp2 products (squarings included) of one step; the two Fp2-by-Fp scalings of a line are 4 Fp products = 4/3
DOUBLING = 12 + 10 + 13 + 4 / 3      # f^2, the doubling step, f * line, the line at P
ADDITION = 13 + 13 + 4 / 3           # the addition step, f * line, the line at P


def products_per_pair(curve):
    k = LOOP[curve]
    dbl, add = k.bit_length() - 1, bin(k).count("1") - 1
    if curve == "bn254":
        return dbl * DOUBLING + (add + 2) * ADDITION + 2   # the two closing lines; pi(Q) is two products
    return dbl * DOUBLING + add * ADDITION


def ladder_products(r):
    k = r - 1
    return 9 * (k.bit_length() - 1) + 14 * (bin(k).count("1") - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[10, 12, 14, 16])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--curves", nargs="+", default=list(CURVES))
    ap.add_argument("--proofs-log-n", type=int, default=12, help="0 skips the verifiers")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairing.json"))
    args = ap.parse_args()

    import gnark_amd
    import pyref
    from gnark_amd import _lib, ecc, g16_verify, groth16
    from gnark_amd.device import affine_words, curve_id
    from helpers import gen_of, pts_to_arr

    results, verifiers = [], []
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
            w1, w2 = affine_words(cid, 0), affine_words(cid, 1)
            rng = np.random.default_rng(0x9A1 + cid)

            def rand_words(m):   # full-width scalars below r: the top word below r's
                w = rng.integers(0, 1 << 64, size=(m, 4), dtype=np.uint64)
                w[:, 3] = rng.integers(1, c.r >> 192, size=m, dtype=np.uint64)
                return w

            def points(group, words):
                return ecc.BatchScalarMultiplication(ctx, curve, group, pts_to_arr(c, group, [gen_of(c, group)]), words, out_device=True)

            for logn in args.log_n:
                n = 1 << logn
                dP, dQ, d_s, out = points(0, rand_words(n)), points(1, rand_words(n)), ctx.to_device(rand_words(n)), ctx.malloc(n * w2 * 8)

                def check():
                    return ecc.PairingCheck(ctx, curve, dP, dQ, n=n)[1:]

                def scale():
                    red = C.c_uint64(0)
                    lib.check(lib.ga_scale_points(ctx.handle, cid, 1, C.c_void_p(dQ.ptr), n, _lib.SCALE_EACH, C.c_void_p(d_s.ptr), 0,
                                                  _lib.SCALARS_ON_DEVICE | _lib.BASES_ON_DEVICE | _lib.RESULT_ON_DEVICE, C.c_void_p(out.ptr), C.byref(red)))
                    return red.value

                runs, ladder = [], []
                for rep in range(args.reps + 1):   # (rep 0 warms both up: the scratch exists afterwards)
                    st, out2 = profiled(check)
                    os.environ["GA_SCALE_WINDOW"] = "0"
                    sl, _ = profiled(scale)
                    os.environ.pop("GA_SCALE_WINDOW", None)
                    if rep:
                        runs.append(st)
                        ladder.append(sl["scale_ladder"])
                    assert out2 == (1, 0), out2   # random pairs: the one group is not 1
                stages = {k: [round(r.get(k, 0.0), 3) for r in runs] for k in ("pairing_miller", "pairing_product", "pairing_final")}
                call_ms = [round(sum(r.get(k, 0.0) for k in stages), 3) for r in runs]
                miller = min(stages["pairing_miller"])
                rec = {"curve": curve, "log_n": logn, "reps": args.reps, "stage_ms": stages, "call_ms": call_ms,
                       "pairs_per_s": round(n / (min(call_ms) * 1e-3)),
                       "fp2_products_per_pair": round(products_per_pair(curve), 1),
                       "miller_fp2_products_per_s": round(n * products_per_pair(curve) / (miller * 1e-3)),
                       "scale_points_g2_plain_ladder": {"ms": [round(v, 3) for v in ladder], "fp2_products_per_point": ladder_products(c.r),
                                                        "fp2_products_per_s": round(n * ladder_products(c.r) / (min(ladder) * 1e-3))}}
                rec["miller_over_ladder_rate"] = round(rec["miller_fp2_products_per_s"] / rec["scale_points_g2_plain_ladder"]["fp2_products_per_s"], 4)
                results.append(rec)
                print("PAIRING_RESULT " + json.dumps(rec), flush=True)
                for b in (dP, dQ, d_s, out):
                    b.free()

            if args.proofs_log_n:
                N, r = 1 << args.proofs_log_n, c.r
                a, b, g, d, k0, k1 = (int(x) % r or 1 for x in np.random.default_rng(0x16 + cid).integers(1, 1 << 62, size=6))
                host = lambda group, ks: points(group, np.array([[(k >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for k in ks], dtype=np.uint64))

                def to_host(buf, m, w):
                    try:
                        return buf.to_host((m, w))
                    finally:
                        buf.free()
                hdr1, hdr2 = to_host(host(0, [a, k0, k1]), 3, w1), to_host(host(1, [b, g, d]), 3, w2)
                vk = g16_verify.VerifyingKey(cid, hdr1[0], hdr2[0], hdr2[1], hdr2[2], hdr1[1:3].copy())
                ints = lambda W: [int.from_bytes(row.tobytes(), "little") for row in W]
                xs, ys, pws = ints(rand_words(N)), ints(rand_words(N)), ints(rand_words(N))
                dinv = pow(d, -1, r)
                zs = [(x * y - a * b - (k0 + pw * k1) * g) * dinv % r for x, y, pw in zip(xs, ys, pws)]
                Ar, Bs, Krs = to_host(host(0, xs), N, w1), to_host(host(1, ys), N, w2), to_host(host(0, zs), N, w1)
                proofs = [groth16.Proof(cid, Ar[i], Bs[i], Krs[i], lib) for i in range(N)]
                witnesses = [[pw] for pw in pws]
                rec = {"curve": curve, "proofs": N, "public_inputs": 1}
                for name, call in (("VerifyMany", lambda: bool(g16_verify.VerifyMany(ctx, vk, proofs, witnesses).all())),
                                   ("BatchVerify", lambda: g16_verify.BatchVerify(ctx, vk, proofs, witnesses, np.random.default_rng(1)))):
                    secs = []
                    for rep in range(args.reps + 1):
                        t0 = time.perf_counter()
                        assert call() is True, name
                        ctx.sync()
                        if rep:
                            secs.append(time.perf_counter() - t0)
                    rec[name] = {"s": [round(v, 4) for v in secs], "proofs_per_s": round(N / min(secs))}
                bad = list(witnesses)
                bad[N // 2] = [(pws[N // 2] + 1) % r]
                assert not g16_verify.BatchVerify(ctx, vk, proofs, bad, np.random.default_rng(1)) and int(g16_verify.VerifyMany(ctx, vk, proofs, bad).sum()) == N - 1
                verifiers.append(rec)
                print("PAIRING_VERIFIERS " + json.dumps(rec), flush=True)
    doc = {"device_results": results, "verifiers": verifiers,
           "products_note": "fp2_products_per_pair is counted from the formulas of pairing.hip.h (squarings count as products, an Fp2-by-Fp scaling as 2/3); "
                            "the ladder's count is 9 products a doubling and 14 an addition on the bits of r - 1.  The verifier times are wall clock and "
                            "include the host side (the arrays of the calls are assembled in Python)",
           "cpu_reference": None, "cpu_reference_note": "gnark-crypto was not available where this was measured: no CPU figure"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

/* gnark_amd.h -- C ABI of libgnark_amd.so, the MI355X (gfx950) prover backend for gnark.
 *
 * This is the drop-in boundary: the surface a Go package `backend/accelerated/mi355x/groth16` binds through
 * cgo in place of the ~20 ICICLE entry points that backend/accelerated/icicle/groth16/bn254/icicle.go uses
 * (reference line numbers below are into /root/reference).  INTEGRATION.md shows the cgo stub.
 *
 * Conventions
 *  - All field elements / points are gnark-crypto memory images: little-endian 64-bit limbs in Montgomery
 *    form (fr.Element = [4]uint64; fp.Element = [4]uint64 BN254 / [6]uint64 BLS12-381 and BLS12-377); G1Affine = {X,Y};
 *    G2Affine = {X{A0,A1}, Y{A0,A1}}; point at infinity = all-zero coordinates; G1Jac/G2Jac = {X,Y,Z}.
 *    A Go slice `[]fr.Element` / `[]curve.G1Affine` can be passed as `unsafe.Pointer(&s[0])` unchanged.
 *  - No pointer passed in is retained after the call returns (cgo pointer rules): inputs are copied to
 *    device memory (or are already device pointers, see GA_*_ON_DEVICE) before the function returns.
 *  - Every entry point selects its device itself (hipSetDevice), so callers need not pin OS threads
 *    (icicle.go relies on RunOnDevice + LockOSThread instead).
 *  - Every function returns GA_OK (0) or a negative error code; ga_last_error() gives the message for the
 *    calling thread.  There is NO CPU fallback: without a usable HIP device ga_ctx_create fails.
 *  - Any host thread may call any entry point on any context at any time; results never depend on the interleaving
 *    (icicle.go:77-86,821-823 keeps a per-device prove mutex for the same guarantee).  Calls on one ga_ctx are serialised by an
 *    internal mutex, with exceptions that only add throughput: a context has four lanes (stream + scratch namespace each).
 *    A Groth16 proof runs on a pair of them -- the witness MSMs on one, its H side (computeH, the Z MSM) on the partner lane
 *    from a helper thread (GA_G16_SPLIT=0 keeps one lane) --, a second ga_g16_prove arriving while the first pair is busy runs
 *    on the second pair beside it, and a second ga_msm_table_run* (the PLONK prover commits from several goroutines) or
 *    ga_g16_h_chain* / ga_g16_h_combine (the pieces of a sharded proof) takes lane 1 (GA_G16_LANES=1 restores strict queueing).
 *    ga_g16_lane_stats says how the proofs of a context were scheduled.
 *  - Destroying an object while other threads are still inside entry points that use it is safe for proving keys:
 *    ga_g16_pk_destroy waits for them (a Go `defer pk.FreeGPUResources()` beside another goroutine's Prove); every other
 *    destroy call must come after the last use, as with any C object.
 */
#ifndef GNARK_AMD_H
#define GNARK_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GA_OK 0
#define GA_ERR_INVALID (-1)   /* bad argument */
#define GA_ERR_HIP (-2)       /* HIP runtime error (message in ga_last_error) */
#define GA_ERR_NOMEM (-3)     /* device allocation failed -- or would have left less than GA_HBM_RESERVE_MB (environment, default
                                 1024) MiB of HBM free: the ROCm runtime allocates the kernels' private segments at dispatch time
                                 and aborts the PROCESS when it cannot, so the library never takes the last gigabyte.  After this
                                 error the context and its keys stay usable. */
#define GA_ERR_STATE (-4)     /* object used in the wrong state */

/* curve ids (ecc.ID analogue).  BN254 and BLS12-381, the two curves of BASELINE.json, are built in full.  BLS12-377 is built for
 * GA_G1 and the scalar field only -- what the PLONK / KZG prover needs (backend/plonk/bls12-377): ga_msm, ga_msm_windows, ga_msm_plan,
 * ga_msm_combine_windows, the ga_msm_table_* calls, ga_jac_add / _to_affine / _scalar_mul, ga_generator_mul, ga_gen_bases(_at),
 * ga_gen_scalars, ga_fr_dot, ga_domain_create with ga_fft(_batch) and ga_compute_h(_batch), the ga_plonk_* calls, ga_kzg_open(_batch),
 * ga_fr_linear_combination, ga_fr_poly_evaluate, ga_fr_vec_mul, ga_fr_batch_invert, ga_hash_to_field, ga_batch_scalar_mul(_plan),
 * ga_kzg_to_lagrange_g1 and ga_check_points.  Every other call that takes a curve id, and every call with GA_G2, answers
 * GA_ERR_INVALID for it with a message that names the curve: its Fp2 is Fp[u]/(u^2 + 5), the library's is u^2 + 1, so G2, the
 * pairing and Groth16 are not built for it. */
#define GA_BN254 0
#define GA_BLS12_381 1
#define GA_BLS12_377 2

/* group ids */
#define GA_G1 0
#define GA_G2 1

/* flags for ga_msm */
#define GA_BASES_ON_DEVICE 0x1u        /* `bases` (ga_kzg_to_lagrange_g1, ga_lagrange_coeffs: `powers_affine`; ga_scale_points,
                                         * ga_sparse_point_sums, ga_check_points: `points_affine`; ga_pairing_check: both point vectors) is a device pointer */
#define GA_SCALARS_ON_DEVICE 0x2u      /* `scalars` is a device pointer */
#define GA_TABLE_BATCHED 0x10u         /* ga_msm_table_create: the table will mostly serve ga_msm_table_run_batch (PLONK's grouped
                                         * commitments over the SRS): plan a narrower window -- k bucket sets make the sort keys
                                         * log2(k) bits wider and the reduction k times larger, which moves the optimum down
                                         * (2^22 points: c = 20 instead of 22, PLONK leg 82.9 -> 79.8 ms; a single run costs +1 %) */
#define GA_SCALARS_MONTGOMERY 0x4u     /* scalars are fr.Element images (Montgomery); else canonical LE integers
                                          (ICICLE's AreScalarsMontgomeryForm, icicle.go:861-863,1232) */
#define GA_RESULT_WINDOW_SUMS 0x8u     /* multi-GPU window sharding: see ga_msm_windows */
#define GA_RESULT_ON_DEVICE 0x20u      /* ga_batch_scalar_mul, ga_kzg_to_lagrange_g1, ga_lagrange_coeffs, ga_scale_points,
                                         * ga_sparse_point_sums: `out_affine` (ga_check_points: `status`; ga_pairing_check: `ok`, `gt`) is a device pointer */
#define GA_CHECK_CURVE_ONLY 0x80u      /* ga_check_points: the curve equation only (IsOnCurve), no subgroup test */
#define GA_RESULT_BITREVERSED 0x40u    /* ga_batch_scalar_mul, ga_sparse_point_sums: result i is written at index bitrev(i, log2 n) */

/* NTT direction / ordering, mirroring gnark-crypto fft.Domain.FFT / FFTInverse (prove.go:362-386) */
#define GA_FFT_FORWARD 0
#define GA_FFT_INVERSE 1
#define GA_DIF 0   /* natural in  -> bit-reversed out */
#define GA_DIT 1   /* bit-reversed in -> natural out  */

typedef struct ga_ctx ga_ctx;         /* one per (process, device) */
typedef struct ga_domain ga_domain;   /* fft.Domain analogue: twiddles for one (curve, cardinality) */
typedef struct ga_g16_pk ga_g16_pk;   /* device-resident Groth16 proving key ("PinToGPU", provingkey.go:37-42) */

/* ---- context ------------------------------------------------------------------------------------------
 * replaces: icicle runtime LoadBackend / CreateDevice / WarmUpDevice (groth16_icicle.go:38-72). */
int ga_device_count(int* count);
int ga_ctx_create(int device, ga_ctx** out);
/* ga_ctx_destroy: every object created on the context (proving keys, builders, domains, tables, PLONK keys) must have been destroyed
 * first and no entry point may be running on it -- the objects keep a plain pointer to their context.  The Go package creates one
 * context per device for the life of the process (internal/ga) and never calls this. */
void ga_ctx_destroy(ga_ctx* ctx);
const char* ga_last_error(void);
const char* ga_version(void);
/* device name / gcn arch / total and free bytes (runtime.GetAvailableMemory, icicle.go:475) */
int ga_device_info(ga_ctx* ctx, char* name, size_t name_len, uint64_t* total_bytes, uint64_t* free_bytes);

/* ---- raw device buffers (DeviceSlice analogue: icicle.go:120,321,...) ---------------------------------*/
int ga_malloc(ga_ctx* ctx, size_t bytes, void** dptr);
int ga_free(ga_ctx* ctx, void* dptr);
int ga_copy_to_device(ga_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int ga_copy_to_host(ga_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int ga_sync(ga_ctx* ctx);

/* ---- multi-scalar multiplication -----------------------------------------------------------------------
 * replaces: G1Jac.MultiExp / G2Jac.MultiExp (prove.go:194,207,227,237,283) and icicle msm.Msm / g2.G2Msm
 * (icicle.go:397,451).  Computes sum_i scalars[i] * bases[i].
 *   bases   : n affine points (Montgomery), host or device pointer per flags
 *   scalars : n fr elements, Montgomery if GA_SCALARS_MONTGOMERY
 *   out_jac : HOST buffer for one Jacobian point {X,Y,Z} (Montgomery) -- castable to curve.G1Jac / G2Jac.
 * (0,0) bases are treated as infinity and zero scalars are skipped, as gnark-crypto does.
 * Jacobian results (here and in every entry point below that returns Jacobian points or partial sums) are group elements: two
 * calls on the same inputs return the same point, but not necessarily the same representative {X,Y,Z} -- from 2^25 (bucket,
 * point) pairs the order in which a bucket's points are added is not fixed (the first sort pass ranks with atomics, msm_sort.hip.h 1b),
 * exactly as gnark-crypto's MultiExp returns a different representative for a different NbTasks.  Affine outputs (proofs,
 * commitments, ga_jac_to_affine of any result) are bit-identical from call to call and from device to device. */
int ga_msm(ga_ctx* ctx, int curve, int group, const void* bases, const void* scalars, size_t n, unsigned flags,
           void* out_jac);

/* Window-sharded variant for multi-GPU partitioning A: only windows [win_lo, win_hi) of the
 * Pippenger decomposition are accumulated; out_windows receives (win_hi - win_lo) Jacobian window sums W_j,
 * and *window_bits / *num_windows describe the decomposition so that the caller can all-gather the sums and
 * Horner-combine them with ga_msm_combine_windows.  win_lo = 0, win_hi = -1 means "all windows". */
int ga_msm_windows(ga_ctx* ctx, int curve, int group, const void* bases, const void* scalars, size_t n,
                   unsigned flags, int win_lo, int win_hi, void* out_windows, int* window_bits, int* num_windows);
/* number of windows / window width ga_msm* will use for an n-point MSM (deterministic in (curve, group, n)) */
int ga_msm_plan(int curve, int group, size_t n, int* window_bits, int* num_windows);
/* result = sum_j 2^(window_bits*j) * windows[j]   (host arithmetic; windows are Jacobian, Montgomery) */
int ga_msm_combine_windows(int curve, int group, const void* windows, int num_windows, int window_bits,
                           void* out_jac);

/* ---- fixed-base batch scalar multiplication --------------------------------------------------------------
 * replaces: curve.BatchScalarMultiplicationG1 / G2 -- all the curve work of groth16.Setup (backend/groth16/bn254/setup.go:233,302)
 * -- and the same primitive over the powers of tau in kzg.NewSRS.  out[i] = [scalars[i]] base.
 *   base    : ONE affine point (Montgomery, (0,0) = infinity), host pointer; any point ON the curve, subgroup or not
 *   scalars : n fr elements; canonical LE 4x64 (< r) as gnark's setup passes them, Montgomery with GA_SCALARS_MONTGOMERY;
 *             host, or device with GA_SCALARS_ON_DEVICE
 *   out     : n affine points in gnark's memory image ((0,0) for a zero scalar or an infinite result);
 *             host, or device with GA_RESULT_ON_DEVICE
 *   GA_RESULT_BITREVERSED : out[bitrev(i, log2 n)] = [scalars[i]] base (setup.go:247 on the Z points); n must be a power of two
 * GA_ERR_INVALID: unknown curve or group, a null pointer with n > 0, a base that is not on the curve, GA_RESULT_BITREVERSED with
 * n not a power of two.  n = 0 is GA_OK and touches nothing.  The window width is deterministic in (curve, n); the environment
 * knobs GA_FIXED_BASE_C (2 .. 20) / GA_FIXED_BASE_CHUNK (at most 2^30) force the width and the number of scalars per pass (tests). */
int ga_batch_scalar_mul(ga_ctx* ctx, int curve, int group, const void* base_affine, const void* scalars, size_t n,
                        unsigned flags, void* out_affine);
/* window width / number of windows ga_batch_scalar_mul will use for n scalars: deterministic in (curve, n), the same for both groups;
 * GA_FIXED_BASE_C, when set, is what it reports */
int ga_batch_scalar_mul_plan(int curve, size_t n, int* window_bits, int* num_windows);

/* ---- kzg.ToLagrangeG1: the SRS in Lagrange form ------------------------------------------------------------
 * replaces: gnark-crypto's kzg.ToLagrangeG1 (ecc/<curve>/kzg), the step between a ceremony SRS and plonk.Setup(ccs, srs, srsLagrange).
 * kzg.ToLagrangeG1: powers[i] = [tau^i]G1, i < n  ->  out[i] = [l_i(tau)]G1, natural order, l_i the Lagrange basis of the size-n
 * domain fft.NewDomain(n) builds (generator = fr_root_of_unity(n)).
 * out[i] = [1/n] * sum_j [w^(-i*j)] powers[j] -- a linear map, defined for ANY n points of the group, (0,0) = infinity in and out.
 *   powers : n affine G1 points (gnark's memory image), host, or device with GA_BASES_ON_DEVICE; never modified
 *   out    : n affine G1 points in gnark's memory image, host, or device with GA_RESULT_ON_DEVICE: usable as `bases` of ga_msm and of
 *            ga_msm_table_create(..., GA_BASES_ON_DEVICE).  The bytes are bit-identical to gnark's.
 * `powers` and `out` must not overlap.  The points are NOT validated (gnark does not validate them either): for points off the
 * curve or outside the subgroup the result is whatever the group law's formulas give.
 * GA_ERR_INVALID: unknown curve, a null pointer with n > 0, n not a power of two, n above 2^28 (BN254) / 2^32 (BLS12-381) / 2^47 (BLS12-377), the
 * two-adicity of r.  n = 0 is GA_OK and touches nothing; n = 1 copies the point.
 * Device scratch, kept by the context: n extended points (128 B each for BN254, 192 B for BLS12-381), n/2 twiddle scalars (32 B each),
 * n/2 + 4 words of redo list, and n affine points (64 / 96 B) of staging when `powers` or `out` is on the host.  GA_ERR_NOMEM when
 * that does not fit (always above n = 2^31); the context stays usable. */
int ga_kzg_to_lagrange_g1(ga_ctx* ctx, int curve, const void* powers_affine, size_t n, unsigned flags, void* out_affine);

/* ---- the point iFFT for G1 and G2: the Lagrange transforms of the Groth16 MPC ceremony --------------------
 * replaces: lagrangeCoeffsG1 / lagrangeCoeffsG2 of backend/groth16/<curve>/mpcsetup (lagrange.go:21-64), which Phase2.Initialize
 * (phase2.go:207-210) runs over G1.Tau, G1.AlphaTau, G1.BetaTau and G2.Tau, and VerifyPhase2 runs again for every verifier.
 * mpcsetup lagrangeCoeffsG1 / lagrangeCoeffsG2 (lagrange.go:21-64): out[i] = [1/n] sum_j [w^(-ij)] powers[j], natural order in and out.
 * group == GA_G1 gives the bytes of ga_kzg_to_lagrange_g1.  Flags, limits on n, aliasing and validation rules as there; the device
 * scratch likewise, with G2 points twice the size of G1 points (256 B extended for BN254, 384 B for BLS12-381).
 * GA_ERR_INVALID additionally for an unknown group. */
int ga_lagrange_coeffs(ga_ctx* ctx, int curve, int group, const void* powers_affine, size_t n, unsigned flags, void* out_affine);

/* ---- per-point scalar multiplication: the curve work of the Groth16 MPC ceremony ---------------------------
 * replaces: the ScalarMultiplication loops of backend/groth16/<curve>/mpcsetup -- SrsCommons.update (phase1.go:104-147: the i-th
 * point of G1.Tau, G2.Tau, G1.AlphaTau, G1.BetaTau times c * tau^i) and Phase2.update (phase2.go:110-135: Z and PKK times 1/delta,
 * SigmaCKK[i] times sigma_i).  out[i] = [s_i] points[i]: n full-width variable-base multiplications, a map and not a sum.
 *   points  : n affine points (gnark's memory image, (0,0) = infinity), host, or device with GA_BASES_ON_DEVICE
 *   out     : n affine points in gnark's memory image, host, or device with GA_RESULT_ON_DEVICE.  out == points (the same pointer
 *             AND the same placement) scales in place, as the reference does; otherwise `points` is never written.  Any other
 *             overlap of the two is the caller's error and is not detected.
 *   scalars : fr elements, canonical LE 4x64 integers, or Montgomery with GA_SCALARS_MONTGOMERY.  A canonical value that is not
 *             below r (any 256-bit integer, r itself included) is reduced mod r.
 *             GA_SCALE_EACH: n of them, host, or device with GA_SCALARS_ON_DEVICE; GA_SCALE_ONE / GA_SCALE_POWERS: 1 / 2, host.
 *   first   : GA_SCALE_POWERS only (0 otherwise): the exponent of point 0 -- the tail G1.Tau[N .. 2N-1) of phase1.go:141-146, or a
 *             caller's own chunking, needs no powers from the host.  first + n must not exceed 2^64.
 *   redone  : may be NULL; receives the number of points that left the fast loop for the complete formulas (points of order <= 8,
 *             a prefix of the scalar hitting +-d P; never points at infinity or zero scalars).  0 for an honest SRS.
 * The bytes are gnark's G1Affine / G2Affine images of the exact group elements, whatever the schedule; a zero scalar or a point at
 * infinity gives (0,0).  The points are NOT validated (ScalarMultiplication does not validate them either): for a point of small
 * order or outside the subgroup the result is still the group law's.
 * GA_ERR_INVALID: unknown curve, group or mode; a null pointer with n > 0; first != 0 outside GA_SCALE_POWERS; GA_SCALARS_ON_DEVICE
 * outside GA_SCALE_EACH; n above 2^32.  n = 0 is GA_OK and touches nothing.
 * Device scratch, kept by the context, per pass of at most GA_SCALE_CHUNK points (default 2^20, at most 2^30): 8 + 1 extended points
 * (128 B each for BN254 G1 .. 384 B for BLS12-381 G2), 32 B of scalar, 4 B of redo list per point, and the staging of whatever is on
 * the host.  GA_ERR_NOMEM when that does not fit: nothing is in flight and the context stays usable.  GA_SCALE_WINDOW=0 runs the
 * plain double-and-add ladder instead of the signed 4-bit windows (same bytes; tools/scale_points_bench.py measures both). */
#define GA_SCALE_EACH   0   /* scalars: n fr elements;              out[i] = [scalars[i]] points[i]          */
#define GA_SCALE_ONE    1   /* scalars: 1 fr element s;             out[i] = [s] points[i]                   */
#define GA_SCALE_POWERS 2   /* scalars: 2 fr elements (c, t);       out[i] = [c * t^(first + i)] points[i]   */
int ga_scale_points(ga_ctx* ctx, int curve, int group, const void* points_affine, size_t n, int mode,
                    const void* scalars, uint64_t first, unsigned flags, void* out_affine, uint64_t* redone);

/* ---- batch curve and subgroup checks: accepting points from somebody else -----------------------------------
 * replaces: G1Affine / G2Affine.IsOnCurve and IsInSubGroup, one call for n points -- what gnark-crypto's default decoder
 * (curve.NewDecoder without NoSubgroupChecks) does for every point of a ProvingKey.ReadFrom (backend/groth16/<curve>/marshal.go:305-312),
 * of every ReadFrom of an mpcsetup phase and of kzg.SRS.ReadFrom, here on a vector that may already sit on the device.
 *   points_affine : n G1Affine / G2Affine memory images, host, or device with GA_BASES_ON_DEVICE; never written.
 *   status        : n bytes, may be NULL; host, or device with GA_RESULT_ON_DEVICE.  status[i] is one of the three values below.
 *   out4          : host, required: {points off the curve, points outside the subgroup, index of the first point that is not OK or
 *                   UINT64_MAX, redone}.
 *   flags         : GA_BASES_ON_DEVICE, GA_RESULT_ON_DEVICE, GA_CHECK_CURVE_ONLY (no subgroup test: IsOnCurve alone).
 * The return value says whether the check RAN, not whether the points are good: GA_OK for any mixture of points.  (0,0) is infinity
 * and OK, as in gnark-crypto.  A coordinate whose image is not below p is GA_POINT_OFF_CURVE, decided before any arithmetic (a dump
 * is raw memory).  The truth is "on the curve and [r]P = O"; it is decided by an identity in the curve's seed x0 -- BN254 G1: the
 * curve equation alone (cofactor 1); BLS12-381 and BLS12-377 G1: P + [x0^2] phi(P) = O; BLS12-381 G2: psi(P) = [x0]P; BN254 G2:
 * [x0 + 1]P + psi([x0]P) + psi^2([x0]P) = psi^3([2 x0]P) -- one or two 64-bit ladders per point instead of a 255-bit one.
 * `redone` counts points that met an exceptional step of the fast formulas (points of small order) and were decided by [r]P with
 * the complete formulas: 0 on honest input, never an error.  GA_CHECK_NAIVE=1 runs the definition instead ([r - 1]P = -P, same bytes;
 * tools/check_points_bench.py measures both).
 * GA_ERR_INVALID: unknown curve or group; a null points_affine with n > 0; a null out4; n above 2^32.  n = 0 gives
 * {0, 0, UINT64_MAX, 0} and touches nothing.  Device scratch, kept by the context, per pass of at most GA_CHECK_CHUNK points (default
 * 2^20, at most 2^30): 5 bytes per point, and the staging of points on the host.  GA_ERR_NOMEM when that does not fit: nothing is in
 * flight and the context stays usable. */
#define GA_POINT_OK              0
#define GA_POINT_OFF_CURVE       1   /* a coordinate image not below p, or y^2 != x^3 + b */
#define GA_POINT_NOT_IN_SUBGROUP 2   /* on the curve, outside the prime-order subgroup */
int ga_check_points(ga_ctx* ctx, int curve, int group, const void* points_affine, size_t n, unsigned flags,
                    uint8_t* status, uint64_t* out4);

/* ---- products of pairings over groups of (G1, G2) pairs ------------------------------------------------------
 * ok[g] = 1 iff prod_{i in group g} e(P_i, Q_i) = 1, else 0: one Miller loop per pair, one final exponentiation per group.
 * replaces: curve.PairingCheck of the Groth16 verifier (backend/groth16/<curve>/verify.go:128-139), pedersen.BatchVerifyMultiVk
 * (verify.go:104-112), kzg.Verify / BatchVerifyMultiPoints, the SameRatio pairings of mpcsetup's Verify, and -- through `gt` --
 * vk.Precompute's e(alpha, beta).
 *   p_affine, q_affine : n G1Affine and n G2Affine memory images; host, or BOTH device with GA_BASES_ON_DEVICE; never written.
 *   group_start        : n_groups + 1 host offsets, group_start[0] = 0, non-decreasing, group_start[n_groups] = n; NULL = one group
 *                        of all n pairs (n_groups must then be 1).  An empty group is 1.
 *   ok                 : n_groups bytes, may be NULL; host, or device with GA_RESULT_ON_DEVICE.
 *   gt                 : may be NULL; n_groups values of 12 fp.Element images in the order of gnark-crypto's E12 struct (C0.B0.A0,
 *                        C0.B0.A1, C0.B1.A0, ..., C1.B2.A1), host or device as `ok`: the group's product of Miller values raised to
 *                        (p^6 - 1)(p^2 + 1) h, with h = 3 (p^4 - p^2 + 1)/r for BLS12-381 and, for BN254, h = l0 + l1 p + l2 p^2 + p^3
 *                        (l2 = 6x0^2 + 1, l1 = -36x0^3 - 18x0^2 - 12x0 + 1, l0 = -36x0^3 - 30x0^2 - 18x0 - 2: a multiple of
 *                        (p^4 - p^2 + 1)/r by a cofactor prime to r).  It is the library's own normalisation of e (BN254: the
 *                        optimal-ate Miller loop over 6x0 + 2; BLS12-381: the loop over |x0|, conjugated): bilinear, non-degenerate
 *                        and consistent with itself -- what vk.e = e(alpha, beta) needs --, NOT promised to equal gnark-crypto's Pair.
 *   out2               : host, required: {groups whose product is not 1, index of the first such group or UINT64_MAX}.
 * The return value says whether the check RAN, not what it found.  A pair with (0,0) on either side contributes 1, as gnark-crypto's
 * MillerLoop skips it.  Points are NOT validated (ga_check_points does that): a pair with a point off the curve or outside its
 * subgroup gives an unspecified ok / gt for ITS group only -- never an error, a fault or a hang, never another group's result.
 * GA_ERR_INVALID, before anything is launched: unknown curve; a null p_affine / q_affine with n > 0; a null out2; a group_start that
 * breaks the rules above; n above 2^32 (n_groups above 2^31 - 1).  n_groups = 0 is GA_OK and touches nothing.  Device scratch, kept
 * by the context: one Fp12 (384 / 576 bytes) per pair of a pass of at most GA_PAIRING_CHUNK pairs (default 2^18), one per group,
 * the partial products of groups longer than 16 pairs, and the staging of host points.  GA_ERR_NOMEM when that does not fit: nothing
 * is in flight and the context stays usable.  Stages in the profiler: pairing_miller, pairing_product, pairing_final. */
int ga_pairing_check(ga_ctx* ctx, int curve, const void* p_affine, const void* q_affine, size_t n,
                     const uint64_t* group_start, size_t n_groups, unsigned flags, uint8_t* ok, void* gt, uint64_t* out2);

/* ---- a sparse Fr matrix applied to a vector of points: the constraint loop of Phase2.Initialize ------------
 * replaces: the loops of Phase2.Initialize in backend/groth16/<curve>/mpcsetup (phase2.go:224-247: every term (coeff, wire) of
 * constraint i adds [coeff] coeffX[i] into out[wire], for A, beta A, B, B2, alpha B and C; :283-300: PKK / VKK / CKK = beta A + alpha B + C;
 * :256-261: Z[i] = Tau[i + n] - Tau[i]), each as the rows of one matrix in CSR form (INTEGRATION.md has the table).
 * out[r] = sum_{k = row_start[r]}^{row_start[r+1]-1} [coeffs[terms[k].cid]] points[terms[k].col],  r < n_rows;  an empty row is (0,0).
 *   terms: nnz pairs of uint32 {cid, col} (the memory image of constraint.Term{CID, VID} with VID holding the column), row-major;
 *   row_start: n_rows + 1 offsets, row_start[0] = 0, row_start[n_rows] = nnz;  coeffs: n_coeffs Fr values (gnark's r1cs.Coefficients).
 *   row_start, terms and coeffs are host memory.  Flags: GA_BASES_ON_DEVICE (points), GA_RESULT_ON_DEVICE, GA_SCALARS_MONTGOMERY
 *   (coeffs are fr.Element images; otherwise any 256-bit integers, reduced), GA_RESULT_BITREVERSED (n_rows a power of two: out[bitrev(r)]).
 *   Points are not validated; input and output must not overlap.  *redone (may be NULL): work items that left the fast formulas.
 * A coefficient is treated by its VALUE: 0 drops the term, +-1 and +-2 cost one addition (and one doubling), anything else one
 * scalar multiplication by min(c, r - c).  A (0,0) point contributes nothing.  The bytes are gnark's affine images of the exact
 * group elements whatever the schedule; `redone` counts products and row segments that met an exceptional addition (a repeated or
 * cancelling operand) and were recomputed with the complete formulas -- 0 for generic inputs, never an error.
 * GA_ERR_INVALID, before anything is launched: unknown curve or group; a null pointer (terms, coeffs and points may be null when
 * nnz = 0); row_start[0] != 0 or row_start decreasing; nnz above 2^32 - 1, n_rows above 2^31 - 1; a cid >= n_coeffs or a
 * col >= n_points; GA_RESULT_BITREVERSED with n_rows not a power of two.  n_rows = 0 is GA_OK and touches nothing.
 * Device scratch, kept by the context: 8 B per term, 12 B per row segment, one extended point per row, per general term and per
 * partial sum of a row longer than GA_SPARSE_SEGMENT (default 16) terms; per pass of at most GA_SPARSE_CHUNK general terms (default
 * 2^20) the ladder's scratch of ga_scale_points; the staging of what is on the host.  GA_ERR_NOMEM when that does not fit: nothing
 * is in flight and the context stays usable.  GA_SPARSE_ORDER=1 sorts the products by coefficient id (same bytes). */
int ga_sparse_point_sums(ga_ctx* ctx, int curve, int group, const void* points_affine, size_t n_points,
                         const uint64_t* row_start, size_t n_rows, const uint32_t* terms,
                         const void* coeffs, size_t n_coeffs, unsigned flags, void* out_affine, uint64_t* redone);

/* ---- the scalar side of groth16.Setup: Fr vectors that never leave the device ------------------------------
 * With these four calls groth16.Setup runs from (toxic waste, R1CS matrices) to a pinned proving key without a scalar or a point
 * crossing PCIe: their outputs feed ga_batch_scalar_mul(..., GA_SCALARS_ON_DEVICE | GA_RESULT_ON_DEVICE), whose outputs feed
 * ga_g16_builder_* / ga_msm_table_create(..., GA_BASES_ON_DEVICE).  INTEGRATION.md ("Setup on the device") has the table.
 * Every Fr vector is 4x64-bit little-endian words per element.  Without GA_SCALARS_MONTGOMERY every input element (vectors,
 * coefficients, scales, tau, (c, t)) is a canonical integer -- any 256-bit value, reduced mod r -- and every output element is canonical
 * and below r: what ga_batch_scalar_mul takes without a flag and what setup.go feeds it.  With GA_SCALARS_MONTGOMERY inputs and outputs
 * are fr.Element images.  All results are exact field elements.  Placement: GA_VECTOR_ON_DEVICE for the input vector (`x`, `v`),
 * GA_RESULT_ON_DEVICE for `out`; everything else is host memory.  GA_ERR_NOMEM (device scratch) leaves nothing in flight and the
 * context usable. */
#define GA_VECTOR_ON_DEVICE GA_BASES_ON_DEVICE   /* ga_fr_sparse_matvec: `x`, ga_fr_compact_nonzero: `v` is a device pointer */

/* replaces: the Lagrange values of setupABC (backend/groth16/bn254/setup.go:356-421: a running product over the domain, then one
 * fr.BatchInvert).  out[i] = L_i(tau), i < m <= n, over the domain fft.NewDomain(n) builds (generator = fr_root_of_unity(n)):
 * L_i = (tau^n - 1) * n^-1 * w^i * inv(tau - w^i) with inv(0) = 0 as fr.BatchInvert leaves zeros -- for tau inside the domain
 * tau^n - 1 = 0 and every output is 0, which is what the reference produces.  tau: one host element.
 * GA_ERR_INVALID: unknown curve; a null pointer with m > 0; n not a power of two or above 2^28 (BN254) / 2^32 (BLS12-381), the
 * two-adicity of r; m > n.  m = 0 is GA_OK and touches nothing.
 * Device scratch, kept by the context: 3 x 32 B per element (differences and the batch inversion's two buffers), and 32 B per element
 * of staging when `out` is on the host. */
int ga_fr_lagrange_at(ga_ctx* ctx, int curve, uint64_t n, const void* tau, size_t m, unsigned flags, void* out);

/* replaces: the term loops of setupABC (setup.go:346-428: every term (coeff, wire) of constraint i adds coeff * L_i(tau) into A[wire],
 * B[wire], C[wire]) and the K loop (:142-178: (beta A + alpha B + C) / delta, or / gamma for public, commitment and private-committed
 * wires), each as the rows of one matrix in CSR form -- the Fr twin of ga_sparse_point_sums, with the same memory image.
 * out[r] = s_r * sum_{k = row_start[r]}^{row_start[r+1]-1} coeffs[terms[k].cid] * x[terms[k].col],  r < n_rows;  an empty row gives 0.
 *   x: n_cols elements, host, or device with GA_VECTOR_ON_DEVICE; terms, row_start, coeffs (n_coeffs elements): as in
 *   ga_sparse_point_sums, host memory;  s_r = row_scales[row_class[r]]: row_class n_rows bytes, row_scales n_classes (1 .. 256)
 *   elements, host; both NULL means s_r = 1.  `x` and `out` must not overlap.  Coefficients are not classified by value: a zero one
 *   contributes zero by arithmetic.
 * GA_ERR_INVALID, before anything is written: unknown curve; a null pointer (x, terms and coeffs may be null when nnz = 0); only one
 * of row_class / row_scales null, or n_classes outside 1 .. 256; row_start[0] != 0 or row_start decreasing; nnz above 2^32 - 1,
 * n_rows above 2^31 - 1; a cid >= n_coeffs, a col >= n_cols or a row_class[r] >= n_classes.  n_rows = 0 is GA_OK and touches nothing.
 * Device scratch, kept by the context: 8 B per term, 12 B per row segment, 32 B per coefficient and per partial sum of a row longer
 * than GA_FR_SPARSE_SEGMENT (environment, default 32) terms, 1 B per row of classes; the staging of what is on the host. */
int ga_fr_sparse_matvec(ga_ctx* ctx, int curve, const void* x, size_t n_cols, const uint64_t* row_start, size_t n_rows,
                        const uint32_t* terms, const void* coeffs, size_t n_coeffs, const uint8_t* row_class,
                        const void* row_scales, size_t n_classes, unsigned flags, void* out);

/* replaces: the zero filter of setup.go:195-219 (A and B lose their zero entries before the point stage; InfinityA / InfinityB
 * remember where they were).  out receives the non-zero elements of v in order -- moved, not converted: zero is zero in both forms --,
 * mask[i] = 1 where v[i] == 0 (host, n bytes, may be NULL), *count = the number kept.  Elements of out past *count are not written.
 * out == v (the same pointer AND the same placement) compacts in place, as the reference does; any other overlap is the caller's error.
 * GA_ERR_INVALID: unknown curve; a null pointer (count always; v, out with n > 0); n above 2^31 - 1.  n = 0 sets *count = 0.
 * Device scratch, kept by the context: 8 B per element and the scan's temporary storage; n bytes of mask; 32 B per element for each
 * of: `v` on the host, `out` on the host or in place. */
int ga_fr_compact_nonzero(ga_ctx* ctx, int curve, const void* v, size_t n, unsigned flags, void* out, uint8_t* mask,
                          uint64_t* count);

/* replaces: the Z scalars of setup.go:181-192 (tau^i * (tau^n - 1) / delta) and the powers of tau of kzg.NewSRS.
 * out[i] = c * t^(first + i), i < n;  scalars: the two elements (c, t), host.  The progression ga_scale_points generates for
 * GA_SCALE_POWERS, written out as a vector.  first + n must not exceed 2^64.
 * GA_ERR_INVALID: unknown curve; a null pointer with n > 0; n above 2^32 or first + n above 2^64.  n = 0 is GA_OK and touches nothing.
 * Device scratch: 32 B per element of staging when `out` is on the host. */
int ga_fr_powers(ga_ctx* ctx, int curve, const void* scalars, uint64_t first, size_t n, unsigned flags, void* out);

/* ---- MSM over pinned bases with precomputed window multiples ---------------------------------------------
 * (ICICLE's MSMConfig.PrecomputeFactor / precompute-bases, icicle.go:507-525.)  ga_msm_table_create uploads (or takes
 * from the device) n affine bases and stores [2^(c*w)]P_i for every window w: windows x n points, sized for the
 * 288 GB of an MI355X (2^24 BN254 G1 points: 12 GiB).  All windows then share one bucket set, so ga_msm_table_run does
 * windows x n bucket additions, ONE bucket reduction and no Horner step.  Results are identical to ga_msm. */
typedef struct ga_msm_table ga_msm_table;
/* flags: GA_BASES_ON_DEVICE, GA_TABLE_BATCHED */
int ga_msm_table_create(ga_ctx* ctx, int curve, int group, const void* bases, size_t n, unsigned flags, ga_msm_table** out);
void ga_msm_table_destroy(ga_msm_table* t);
/* scalars: exactly n fr elements (the table's n); flags: GA_SCALARS_ON_DEVICE, GA_SCALARS_MONTGOMERY */
int ga_msm_table_run(ga_msm_table* t, const void* scalars, unsigned flags, void* out_jac);
int ga_msm_table_info(ga_msm_table* t, int* window_bits, int* num_windows, uint64_t* table_bytes);
/* windows [win_lo, win_hi) of the table only (multi-GPU partition A on pinned bases): the 2^(c*w) factors are part of the table,
 * so the Jacobian results of disjoint window ranges ADD UP to ga_msm_table_run's result (ga_jac_add); no Horner step.  An empty
 * range gives the point at infinity. */
int ga_msm_table_run_windows(ga_msm_table* t, const void* scalars, unsigned flags, int win_lo, int win_hi, void* out_jac);
/* k scalar vectors (1 <= k <= 16; scalars[j] -> n field elements each, all host or all device as `flags` says) over the SAME pinned
 * bases in ONE pass: one sort, one task list, one launch sequence, k bucket sets; out_jacs receives k Jacobian points in order.
 * What the three wire commitments [L],[R],[O] and the three quotient shards [H0],[H1],[H2] of a PLONK proof call
 * (backend/plonk/bn254/prove.go:404-489,558-633: three kzg.Commit on the same SRS issued together): the latency-bound tails of
 * an MSM (bucket reduction, task building) are paid once per batch instead of once per polynomial. */
int ga_msm_table_run_batch(ga_msm_table* t, const void* const* scalars, uint32_t k, unsigned flags, void* out_jacs);

/* ---- small host-side group helpers used by the Go epilogue / multi-GPU combine -------------------------
 * (curve.G1Jac.AddAssign / ScalarMultiplication / FromJacobian, prove.go:199-292).  Host arithmetic. */
int ga_jac_add(int curve, int group, const void* a_jac, const void* b_jac, void* out_jac);
int ga_jac_to_affine(int curve, int group, const void* a_jac, void* out_affine);
int ga_jac_scalar_mul(int curve, int group, const void* a_jac, const void* scalar_canonical_le32,
                      void* out_jac);

/* ---- NTT -----------------------------------------------------------------------------------------------
 * replaces: fft.NewDomain (setup.go:101), fft.Domain.FFT / FFTInverse (prove.go:362-368,386) and icicle
 * ntt.InitDomain / ntt.Ntt (icicle.go:163,1425,1428,1474). */
int ga_domain_create(ga_ctx* ctx, int curve, uint64_t cardinality, ga_domain** out);
void ga_domain_destroy(ga_domain* d);
/* In-place transform of `cardinality` fr elements (Montgomery).  direction: GA_FFT_FORWARD / GA_FFT_INVERSE
 * (inverse includes the 1/n factor); decimation: GA_DIF / GA_DIT; on_coset: fft.OnCoset() with the domain's
 * FrMultiplicativeGen (5 for BN254, 7 for BLS12-381, 22 for BLS12-377).  data is a host pointer unless on_device != 0. */
int ga_fft(ga_domain* d, void* data, int direction, int decimation, int on_coset, int on_device);
/* `count` transforms of one size in one call: data = count vectors of `cardinality` fr elements, contiguous; the other arguments
 * as ga_fft's, the same for every vector.  Replaces a loop of fft.Domain.FFT / FFTInverse over vectors of one domain (the three
 * chains of computeH, prove.go:362-368; PLONK's L, R, O and h1..h3): every pass of the transform is ONE launch over all the
 * vectors, so small transforms (one workgroup per launch at 2^10) fill the device together.  Vector j's result is ga_fft's on vector
 * j alone, bit for bit.  count = 0 is GA_OK and touches nothing. */
int ga_fft_batch(ga_domain* d, void* data, uint32_t count, int direction, int decimation, int on_coset, int on_device);

/* computeH (prove.go:346-389 / icicle.go:1391-1488): h = coefficients of (A*B - C)/(X^n - 1) in bit-reversed
 * order.  a,b,c hold n_constraints fr elements (Montgomery), zero-padded internally to the domain size;
 * h_out receives cardinality elements.  Pointers are host unless on_device != 0 (then a is clobbered). */
int ga_compute_h(ga_domain* d, const void* a, const void* b, const void* c, uint64_t n_constraints,
                 void* h_out, int on_device);
/* computeH for `count` solutions of one circuit (a loop of prove.go:346-389 over the solutions): a, b, c = [count][n_constraints]
 * contiguous; h_out = [count][cardinality], each h as ga_compute_h's for its triple, bit for bit.  The seven transforms are batched
 * launch chains (ga_fft_batch) and the point-wise step is one launch.  Pointers are host unless on_device != 0 (a, b, c are left
 * untouched either way).  count = 0 is GA_OK and touches nothing. */
int ga_compute_h_batch(ga_domain* d, const void* a, const void* b, const void* c, uint32_t count, uint64_t n_constraints,
                       void* h_out, int on_device);

/* ---- PLONK: quotient and grand product on the device ---------------------------------------
 * replaces: (*instance).computeNumerator + divideByZH (backend/plonk/bn254/prove.go:841-1123,1287-1350; the "we do **a lot** of
 * FFT here" loop, ~108 FFTs of size n on the CPU) and iop.BuildRatioCopyConstraint (gnark-crypto, call site prove.go:645-655).
 * domain0 / domain1 are ga_domain handles of cardinality n and rho*n (rho = 4, or 8 below 6 constraints, prove.go:247-251).
 * Every polynomial is n fr elements (Montgomery), either canonical coefficients in regular order or -- when its bit of
 * lagrange_mask is set -- evaluations on domain0 in regular order (what s.x[...] holds before computeNumerator).  Bit order:
 * L R O Z Ql Qr Qm Qo Qk S1 S2 S3, then Qcp_0, Pi2_0, Qcp_1, Pi2_1, ...  (prove.go:44-59 without ZS, which is Z shifted).
 * bl, br, bo: the blinding polynomials of L, R, O (order 1: 2 coefficients), bz: of Z (order 2: 3 coefficients), prove.go:72-75.
 * h_out: rho*n fr elements, canonical, regular order -- s.h after divideByZH; h1/h2/h3 are its slices (prove.go:691-728). */
#define GA_PLONK_ON_DEVICE 0x1u   /* polynomials and the output are device pointers */
typedef struct ga_plonk_quotient_in {
    uint32_t nb_bsb;                     /* len(proof.Bsb22Commitments), at most 16 */
    const void *l, *r, *o, *z, *ql, *qr, *qm, *qo, *qk, *s1, *s2, *s3;
    const void* const* qcp;              /* [nb_bsb] s.trace.Qcp[i] */
    const void* const* pi2;              /* [nb_bsb] s.cCommitments[i] */
    uint64_t lagrange_mask;
    const void *bl, *br, *bo, *bz;
    const void *alpha, *beta, *gamma;    /* fr, Montgomery */
    uint32_t flags;
} ga_plonk_quotient_in;
int ga_plonk_quotient(ga_domain* domain0, ga_domain* domain1, const ga_plonk_quotient_in* in, void* h_out);
/* The circuit-constant half of the quotient pinned in HBM -- the precomputation prove.go:1030-1034 rules out on a CPU ("we could
 * pre-compute these rho*2 FFTs and store them at the cost of a huge memory footprint"): the evaluations of Ql, Qr, Qm, Qo, S1,
 * S2, S3 and every Qcp_i on each of the rho cosets, plus 1/(x-1) on each coset: (8 + nb_bsb) * rho * n * 32 bytes (4.3 GB at
 * n = 2^22).  ga_plonk_pk_create reads only ql, qr, qm, qo, s1, s2, s3, qcp, nb_bsb, lagrange_mask and flags of `in`;
 * ga_plonk_quotient_pinned reads only l, r, o, z, qk, pi2, the blinding polynomials, the challenges, lagrange_mask and flags
 * (6 + nb_bsb inverse/forward transform chains per proof instead of 12 + 2*nb_bsb).  The domains must outlive the key. */
typedef struct ga_plonk_pk ga_plonk_pk;
int ga_plonk_pk_create(ga_domain* domain0, ga_domain* domain1, const ga_plonk_quotient_in* in, ga_plonk_pk** out);
void ga_plonk_pk_destroy(ga_plonk_pk* pk);
int ga_plonk_quotient_pinned(ga_plonk_pk* pk, const ga_plonk_quotient_in* in, void* h_out);
/* Z in Lagrange form, regular order (n elements): Z[0] = 1, Z[i+1] = Z[i] * prod_k (e_k[i] + beta*id_k(i) + gamma) /
 * prod_k (e_k[i] + beta*id(perm[k*n+i]) + gamma), id over {1, g, g^2} * w^i.  l, r, o: evaluations on domain0; permutation:
 * 3n int64 (s.trace.S). */
int ga_plonk_build_z(ga_domain* domain0, const void* l, const void* r, const void* o, const int64_t* permutation,
                     const void* beta, const void* gamma, int on_device, void* z_out);
/* kzg.Open(p, point, pk) -> OpeningProof{H, ClaimedValue} (gnark-crypto kzg, call sites backend/plonk/bn254/prove.go:681,788,827):
 * claimed value p(point) and H = commitment to (p(X) - p(point)) / (X - point) over the pinned monomial SRS.  The reference's
 * division is a sequential Horner recurrence on the CPU; here it is a scaling, a suffix sum and a scaling on the device, followed
 * by the table MSM.  srs: ga_msm_table over pk.Kzg.G1 with at least len(p) - 1 points; poly: n fr coefficients (Montgomery; device
 * pointer with GA_SCALARS_ON_DEVICE); point, claimed_value_out: fr Montgomery; h_out: G1Jac. */
int ga_kzg_open(ga_msm_table* srs, const void* poly, size_t n, unsigned flags, const void* point, void* claimed_value_out, void* h_out);

/* ---- PLONK: the same three calls for MANY proofs of ONE circuit (one key, many witnesses) -------------------------------------
 * A proof of 2^10 .. 2^16 gates cannot fill the device: each of the calls above is a chain of small launches with host-built
 * tables and a closing synchronisation, paid once per proof by a service that proves per-transaction instances under one key.
 * The batched forms take `count` proofs per call; the proof is the grid's y dimension of every kernel, the per-proof challenges
 * and blinding terms come from a device array, the scans are segmented per proof and the power tables are built on the device.
 * (Wire and quotient commitments of a batch already have ga_msm_table_run_batch, the transforms ga_fft_batch.)
 * Measured on one MI355X, 16 proofs, operands on the device, against a loop of the single calls (profiles/plonk_batch.json): the three
 * calls together take 0.13 ms per proof against 3.07 at 2^10 gates (BN254), 0.60 against 4.06 at 2^16; none is slower than its loop.
 * Shared rules:
 *   - count = 0 is GA_OK and touches nothing;
 *   - GA_ERR_INVALID, with ga_last_error text, before anything is launched: a null pointer, structs that disagree, and whatever
 *     the single call refuses;
 *   - the proofs go through the device in passes of at most GA_PLONK_BATCH_MAX (environment, 1 .. 16, default 16: the limit of
 *     ga_msm_table_run_batch); a pass that runs out of device memory, when it reserves its scratch or later, is run again with half
 *     as many proofs (its outputs are written last), and GA_ERR_NOMEM comes back only when one proof does not fit; the context stays
 *     usable after it.  One host synchronisation per pass -- an opening's is the one of its table MSM -- and one more per call where
 *     a device-resident permutation is range-checked;
 *   - GA_ERR_HIP for a failed launch or copy; no exception crosses the call (an allocation failure on the host is GA_ERR_NOMEM).
 *
 * ga_plonk_build_z_batch replaces a loop over proofs of iop.BuildRatioCopyConstraint (call site backend/plonk/bn254/prove.go:645-655).
 * l, r, o = [count][n] evaluations on domain0 (regular order), contiguous; permutation: 3n int64, shared (s.trace.S); betas, gammas:
 * count fr each (Montgomery, HOST memory always); z_out = [count][n].  on_device: l, r, o, permutation and z_out are device pointers.
 * Row j is ga_plonk_build_z's result for (l[j], r[j], o[j], betas[j], gammas[j]), bit for bit.  A permutation entry outside [0, 3n)
 * is GA_ERR_INVALID (checked on the host, or by a kernel for a device-resident permutation), as in the single call. */
int ga_plonk_build_z_batch(ga_domain* domain0, const void* l, const void* r, const void* o, const int64_t* permutation,
                           const void* betas, const void* gammas, uint32_t count, int on_device, void* z_out);
/* ga_plonk_quotient_pinned_batch replaces a loop over proofs of computeNumerator + divideByZH (prove.go:841-1123,1287-1350).
 * ins: count structs, each read as ga_plonk_quotient_pinned reads its `in`; all must carry the same nb_bsb (the key's), lagrange_mask
 * and flags, else GA_ERR_INVALID.  h_out = [count][rho*n] (a device pointer with GA_PLONK_ON_DEVICE); block j is
 * ga_plonk_quotient_pinned(pk, &ins[j]) bit for bit.  Per coset ONE coset transform covers the count * (5 + nb_bsb) per-proof
 * polynomials, and ONE inverse transform of size rho*n covers the count quotients. */
int ga_plonk_quotient_pinned_batch(ga_plonk_pk* pk, const ga_plonk_quotient_in* ins, uint32_t count, void* h_out);
/* ga_kzg_open_batch replaces a loop over proofs of kzg.Open (call sites prove.go:681,788,827).  polys: count pointers to n fr
 * coefficients each (all host, or all device with GA_SCALARS_ON_DEVICE); points: count fr (Montgomery, host); claimed_values_out:
 * count fr (host); h_out: count G1Jac (host).  Item j is ga_kzg_open's result for (polys[j], points[j]): the claimed value bit for
 * bit, H the same group element (a Jacobian representative, as everywhere).  The count quotients go through the batched table MSM
 * in one pass.  GA_ERR_INVALID: a null entry of polys, n = 0, a table that is not G1 or holds fewer than n - 1 points, or count
 * passes of the table's size beyond the 2^31 pair index space of ga_msm_table_run_batch. */
int ga_kzg_open_batch(ga_msm_table* srs, const void* const* polys, size_t n, uint32_t count, unsigned flags, const void* points,
                      void* claimed_values_out, void* h_out);
/* out[i] = sum_{j<k} scalars[j] * vecs[j][i], k <= 16 per call: the polynomial folding of kzg.BatchOpenSinglePoint and the
 * linear combinations of innerComputeLinearizedPoly (backend/plonk/bn254/prove.go:1352-1460) in one pass.  scalars: k fr
 * (Montgomery, host); vecs/out: n fr each, all host or all device (on_device). */
int ga_fr_linear_combination(ga_ctx* ctx, int curve, uint64_t n, int k, const void* const* vecs, const void* scalars, void* out,
                             int on_device);
/* p(point) of a canonical-form polynomial (iop.Polynomial.Evaluate, evaluateBlinded prove.go:1186-1215). */
int ga_fr_poly_evaluate(ga_ctx* ctx, int curve, const void* poly, uint64_t n, const void* point, void* value_out, int on_device);
/* out[i] = a[i] * b[i] over fr (fr.Vector.Mul of gnark-crypto; ICICLE's vecOps Mul of icicle.go:1453-1458).  All host or all
 * device pointers (on_device); out may alias a or b. */
int ga_fr_vec_mul(ga_ctx* ctx, int curve, const void* a, const void* b, size_t n, void* out, int on_device);
/* fr.BatchInvert in place (zeros stay zero): the batchInvert of prove.go:1134-1147 */
int ga_fr_batch_invert(ga_ctx* ctx, int curve, void* v, uint64_t n, int on_device);

/* ---- PLONK: verification of MANY proofs under one key ---------------------------------------------------------
 * replaces: the arithmetic of plonk.Verify (backend/plonk/bn254/verify.go:124-318) for `count` proofs at once: PI(zeta) over the public
 * inputs and the BSB22 hashes (:136-188), the algebraic relation constLin == ClaimedValues[0] (:206-223), the scalars of the
 * linearised digest (:225-277), kzg.FoldProof and kzg.BatchVerifyMultiPoints (:282-318), and the subgroup tests of :61-85.
 * NOT replaced -- the caller supplies them: the Fiat-Shamir challenges gamma, beta, alpha, zeta (gnark-crypto's fiatshamir
 * transcript), the fold challenge v of kzg.FoldProof's transcript, the scalar u that BatchVerifyMultiPoints draws from crypto/rand,
 * and the hashed BSB22 commitments (ga_hash_to_field with DST "BSB22-Plonk" over the marshalled commitments, :162-175).
 *
 * The key: the points of plonk.VerifyingKey on the device; Size, SizeInv, Generator and CosetShift are domain0's, and so is the
 * curve (BN254 or BLS12-381; a BLS12-377 domain is refused by name: no pairing).  Everything behind `in` is host memory and is
 * copied; the domain must outlive the key.  GA_ERR_INVALID: a null pointer (commitment_constraint_indexes and qcp may be null
 * when nb_bsb = 0), nb_bsb above 16, nb_public + nb_bsb above the domain's size, a constraint index that puts its term at or
 * beyond the size. */
typedef struct ga_plonk_vk ga_plonk_vk;
typedef struct ga_plonk_vk_in {
    uint64_t nb_public;                              /* vk.NbPublicVariables */
    uint32_t nb_bsb;                                 /* len(vk.Qcp), at most 16 */
    const uint64_t* commitment_constraint_indexes;   /* nb_bsb */
    const void *ql, *qr, *qm, *qo, *qk, *s1, *s2, *s3;   /* G1Affine each (vk.S[0..2]) */
    const void* qcp;                                 /* nb_bsb G1Affine, contiguous */
    const void* kzg_g1;                              /* vk.Kzg.G1 */
    const void* kzg_g2;                              /* vk.Kzg.G2[0], G2[1]: two G2Affine, contiguous */
} ga_plonk_vk_in;
int ga_plonk_vk_create(ga_domain* domain0, const ga_plonk_vk_in* in, ga_plonk_vk** out);
void ga_plonk_vk_destroy(ga_plonk_vk* vk);

/* `count` proofs as five arrays; every fr is a Montgomery image below r (gnark's fr.Element), every point a G1Affine image.
 * Host memory, or ALL device memory with GA_PLONK_ON_DEVICE (then rows_out, ok and relation_ok are device pointers too; weights
 * and out2 are always host).  public_inputs / bsb_hashes may be null when nb_public / nb_bsb is 0. */
typedef struct ga_plonk_proofs {
    const void* points;        /* [count][9 + nb_bsb] G1Affine: L R O Z H0 H1 H2 W_zeta W_zeta_omega Bsb_0.. */
    const void* evals;         /* [count][7 + nb_bsb] fr: ClaimedValues[0 .. 5 + nb_bsb], then ZShiftedOpening.ClaimedValue */
    const void* challenges;    /* [count][6] fr: gamma beta alpha zeta v u */
    const void* public_inputs; /* [count][nb_public] fr */
    const void* bsb_hashes;    /* [count][nb_bsb] fr: the hashed commitments of verify.go:171-175 */
} ga_plonk_proofs;
#define GA_PLONK_VERIFY_COMBINED       0x2u   /* one randomised check of all proofs instead of one verdict each */
#define GA_PLONK_VERIFY_NO_POINT_CHECK 0x4u   /* the caller has run the subgroup tests of verify.go:61-85 itself */
/* The scalar side alone: relation_ok[j] = (constLin == ClaimedValues[0]) of proof j, and rows_out = [count][2 (9 + nb_bsb) + 2] fr,
 * row j the coefficients of proof j's whole KZG check e(P_j, G2[0]) e(Q_j, G2[1]) = 1 with (E = sum_k v^k ClaimedValues[k], zu the
 * shifted claimed value, D0 the linearised digest, F = D0 + v L + v^2 R + v^3 O + v^4 S1 + v^5 S2 + sum_t v^(6+t) Qcp_t)
 *     P_j = F - E G1 + zeta W_zeta + u (Z - zu G1 + omega zeta W_zeta_omega),      Q_j = -(W_zeta + u W_zeta_omega)
 * in the column order   G1 Ql Qr Qm Qo Qk S1 S2 S3 Qcp_0..  |  L R O Z H0 H1 H2 W_zeta W_zeta_omega Bsb_0..  |  -1, -u
 * (key points, proof points, the two coefficients of Q_j) -- what a caller with its own MSM needs.  The inverse of 0 is 0, as
 * fr.Inverse / BatchInvert / Div have it: zeta on the domain gives what verify.go computes.  Two launches (profiler stages
 * plonk_vf_public, plonk_vf_rows) and one host synchronisation. */
int ga_plonk_verify_scalars(ga_plonk_vk* vk, const ga_plonk_proofs* p, uint32_t count, unsigned flags, void* rows_out,
                            uint8_t* relation_ok);
/* The whole verifier.  Default: ga_check_points' tests on the count * (9 + nb_bsb) proof points (unless NO_POINT_CHECK), the rows,
 * P_j and Q_j of every proof as the 2 count rows of one sparse point sum over [key points | proof points], and ONE pairing pass of
 * count groups of two pairs:  ok[j] = relation_ok[j] && every point of proof j passed && the pairing product of group j is 1.
 * out2 = {proofs rejected, index of the first one or UINT64_MAX}; relation_ok may be NULL.
 * GA_PLONK_VERIFY_COMBINED: weights = count fr (Montgomery, host) chosen by the caller -- the randomness of the batch.  The
 * key columns are summed over the proofs with the weights (stage plonk_vf_combine), the proof columns scaled, and
 * P = sum_j rho_j P_j, Q = sum_j rho_j Q_j come from one MSM each; one pairing group.  ok[0] = every relation and every point
 * check passed and e(P, G2[0]) e(Q, G2[1]) = 1; out2 = {0 or 1, 0 or UINT64_MAX}; relation_ok stays per proof.
 * The return value says whether the check RAN, not what it found: a bad point is a rejected proof (its terms are left out of the
 * sums), never an error and never another proof's verdict.  count = 0 is GA_OK and touches nothing.  GA_ERR_INVALID, before any
 * launch: a null pointer, count above 2^20, combined mode without weights, a null out2.  Device scratch comes from the context;
 * GA_ERR_NOMEM leaves nothing in flight and the context usable.  Host synchronisations: those of the point check, the sparse sum
 * or the two MSMs, and the pairing, plus ONE for the rows (the sparse sum classifies its coefficients on the host). */
int ga_plonk_verify(ga_plonk_vk* vk, const ga_plonk_proofs* p, uint32_t count, unsigned flags, const void* weights, uint8_t* ok,
                    uint8_t* relation_ok, uint64_t* out2);

/* ---- Groth16 -------------------------------------------------------------------------------------------
 * replaces: (*ProvingKey).setupDevicePointers (icicle.go:88-264) and Prove (icicle.go:784-1360).
 * ga_g16_key describes gnark's groth16 ProvingKey (setup.go:25-48) by pointer+length; everything is copied to
 * the device synchronously by ga_g16_pk_create. */
typedef struct ga_g16_key {
    int curve;
    uint64_t domain_cardinality;     /* pk.Domain.Cardinality */
    const void* g1_alpha;            /* G1Affine */
    const void* g1_beta;
    const void* g1_delta;
    const void* g1_a; uint64_t len_a;   /* pk.G1.A (infinity entries removed, setup.go:195-219) */
    const void* g1_b; uint64_t len_b;   /* pk.G1.B */
    const void* g1_z; uint64_t len_z;   /* pk.G1.Z, bit-reversed, len n-1 (setup.go:247-249) */
    const void* g1_k; uint64_t len_k;   /* pk.G1.K */
    const void* g2_beta;             /* G2Affine */
    const void* g2_delta;
    const void* g2_b; uint64_t len_b2;  /* pk.G2.B */
    const uint8_t* infinity_a;       /* pk.InfinityA as bytes (Go []bool image), len nb_wires */
    const uint8_t* infinity_b;
    uint64_t nb_wires;
    uint64_t nb_infinity_a;
    uint64_t nb_infinity_b;
    int32_t precompute;              /* 0: precompute window tables for A,B,K,Z,G2.B -- those that fit comfortably in free HBM, see ga_g16_table_layout
                                        (default), 1: always, -1: never */
    uint32_t shard_index;            /* multi-GPU partition B: pin only slice shard_index of shard_count of every */
    uint32_t shard_count;            /* base vector (contiguous ranges); 0 or 1 = the whole key */
    /* BSB22 commitments (setup.go:260-287, prove.go:60-135,231-235); all zero / NULL for a circuit without api.Commit */
    uint32_t nb_commitments;             /* len(pk.CommitmentKeys) */
    const void* const* ck_basis;         /* [nb_commitments] -> pk.CommitmentKeys[i].Basis (G1Affine) */
    const void* const* ck_basis_exp_sigma; /* [nb_commitments] -> pk.CommitmentKeys[i].BasisExpSigma */
    const uint64_t* ck_len;              /* [nb_commitments] number of points in each basis */
    const uint64_t* k_remove;            /* sorted wire ids left out of the K MSM: every PrivateCommitted wire and every */
    uint64_t len_k_remove;               /* commitment wire (the toRemove list of prove.go:233-235); len_k = nbWires - nbPublic - len_k_remove */
    /* multi-GPU partition A (BASELINE config 4 "window-sharded"): the WHOLE key is pinned on every device and this one
     * accumulates share window_shard_index of window_shard_count of the Pippenger windows of every MSM -- on the pinned window
     * tables, where the 2^(c*w) factors are part of the table, so the partial results of the devices simply add.  0 / 0 or 0 / 1 =
     * all windows.  Not combinable with shard_count > 1. */
    uint32_t window_shard_index;
    uint32_t window_shard_count;
} ga_g16_key;

int ga_g16_pk_create(ga_ctx* ctx, const ga_g16_key* key, ga_g16_pk** out);
/* One proof on a key that is not kept on the device -- the default of the reference's GPU backend (PinToGPU false: the key is uploaded
 * for every proof, icicle.go:797-805) and of the Go package here.  The key (key->precompute is ignored: plain vectors, no tables; whole
 * key, no commitments needed before the proof) is uploaded by a helper thread WHILE the proof runs, each MSM waiting for its own vector
 * only, and dropped before the call returns: its five vector buffers go back to the context's spare set for the next one-shot key
 * (GA_DOMAIN_SPARE); proof bytes identical to ga_g16_pk_create + ga_g16_prove + ga_g16_pk_destroy.  Arguments
 * after `key` as ga_g16_prove.  No pointer is retained after the call. */
int ga_g16_prove_oneshot(ga_ctx* ctx, const ga_g16_key* key, const void* w, const void* a, const void* b, const void* c,
                         uint64_t n_constraints, uint64_t nb_public, const void* r, const void* s, void* proof_out);
void ga_g16_pk_destroy(ga_g16_pk* pk);   /* FreeGPUResources, icicle.go:1493-1549; waits for entry points still using the key */
/* How the ga_g16_prove calls of a context were scheduled since it was created: out6[0] on lanes 0/1 (device free), [1] on lanes
 * 2/3 beside another proof, [2] staged + queued for the device, [3] proofs whose H side ran on a partner lane; [4], [5] = bytes of
 * device scratch held by lanes 0/1 and by lanes 2/3. */
int ga_g16_lane_stats(ga_ctx* ctx, uint64_t* out6);

/* The same key, staged vector by vector (replaces loadG1 / loadG1Raw / loadG2, icicle.go:319-359, one call per host slice).
 * Every call takes ONE flat pointer to pointer-free memory and has copied what it needs when it returns, so a cgo caller never
 * stores a Go pointer inside a C struct and nothing is retained (ga_g16_key holds pointers: from Go it needs runtime.Pinner,
 * see go/backend/accelerated/mi355x).  It is also what the key-file readers below are built on.
 *   create -> reserve(which, len) -> append(which, chunk, count)* -> set_point x5 -> set_infinity x2
 *          [-> add_commitment_key* -> set_k_remove] -> finish  (finish consumes the builder; destroy abandons it) */
/* (ga_g16_builder_append with points == NULL skips `count` points that lie wholly OUTSIDE this shard's slice of the vector: a
 * caller that holds only its own slice -- a file reader seeking past the rest, a rank generating its shard -- need not produce them) */
#define GA_KEY_G1_A 0
#define GA_KEY_G1_B 1
#define GA_KEY_G1_Z 2
#define GA_KEY_G1_K 3
#define GA_KEY_G2_B 4
#define GA_KEY_NB_VECTORS 5
#define GA_KEY_G1_ALPHA 0
#define GA_KEY_G1_BETA 1
#define GA_KEY_G1_DELTA 2
#define GA_KEY_G2_BETA 3
#define GA_KEY_G2_DELTA 4
#define GA_KEY_NB_POINTS 5
typedef struct ga_g16_builder ga_g16_builder;
int ga_g16_builder_create(ga_ctx* ctx, int curve, uint64_t domain_cardinality, uint64_t nb_wires, uint32_t shard_index,
                          uint32_t shard_count, ga_g16_builder** out);
int ga_g16_builder_reserve(ga_g16_builder* b, int which_vector, uint64_t total_len);
/* the next `count` points of vector `which_vector` (affine, Montgomery); with a sharded builder only the part inside this shard's
 * range is copied, the caller still streams the whole vector */
int ga_g16_builder_append(ga_g16_builder* b, int which_vector, const void* points, uint64_t count);
int ga_g16_builder_set_point(ga_g16_builder* b, int which_point, const void* affine);
int ga_g16_builder_set_infinity(ga_g16_builder* b, int which /* 0: InfinityA, 1: InfinityB */, const uint8_t* mask, uint64_t nb_wires);
int ga_g16_builder_add_commitment_key(ga_g16_builder* b, const void* basis, const void* basis_exp_sigma, uint64_t len);
int ga_g16_builder_set_k_remove(ga_g16_builder* b, const uint64_t* wire_ids, uint64_t len);
int ga_g16_builder_set_window_shard(ga_g16_builder* b, uint32_t index, uint32_t count);   /* partition A, see ga_g16_key */
int ga_g16_builder_finish(ga_g16_builder* b, int32_t precompute, ga_g16_pk** out);
void ga_g16_builder_destroy(ga_g16_builder* b);

/* One proof, from the solver's output to the three proof points (prove.go:130-315 minus commitments):
 *   w        : solution.W, nb_wires fr elements (Montgomery)
 *   a,b,c    : solution.A/B/C, n_constraints elements each
 *   nb_public: r1cs.GetNbPublicVariables() (includes the constant-one wire; K scalars start there, prove.go:235)
 *   r,s      : the prover's randomness as fr elements in Montgomery form (prove.go:171-177 samples them; the Go
 *              shim samples and passes them so that tests can inject fixed values)
 *   proof_out: Ar (G1Affine) | Bs (G2Affine) | Krs (G1Affine), Montgomery -- castable to the Proof fields.
 * All pointers are host pointers. */
int ga_g16_prove(ga_g16_pk* pk, const void* w, const void* a, const void* b, const void* c,
                 uint64_t n_constraints, uint64_t nb_public, const void* r, const void* s, void* proof_out);

/* `count` proofs under one key in one device pass: what a loop of groth16.Prove over one ProvingKey computes (prove.go:130-315; the
 * reference has no batch entry point).  For callers that prove many instances of one small circuit, where a single proof is bound by
 * launch chains and host round trips, not by device work.
 *   w, a, b, c: host arrays of `count` host pointers (as ga_msm_table_run_batch takes its scalars): w[j] -> nb_wires elements,
 *               a[j], b[j], c[j] -> n_constraints elements each
 *   r, s      : count fr elements each (Montgomery): the randomness of proof j is (r[j], s[j])
 *   proofs_out: count images Ar | Bs | Krs as ga_g16_prove writes one; proof j is byte-identical to ga_g16_prove's for solution j
 * Solutions go through the device in chunks of at most 16 (GA_G16_BATCH_MAX; fewer when the (scalar, window) pair space or the free
 * HBM asks for it; `count` itself is not limited): the H side of a chunk runs as batched transforms, every MSM over a precomputed
 * table takes the chunk's scalar vectors in one pass, and the host epilogues run beside each other on up to 8 threads.  A base vector
 * WITHOUT a table (a key pinned with precompute = -1, or a partial table set) has no batch path: its MSMs are looped over the
 * solutions -- a batch on such a key is correct, not fast.  The call holds the device like one ga_g16_prove caller (lanes 0/1);
 * a concurrent ga_g16_prove runs beside it on lanes 2/3.  A key that holds a share of a sharded key is refused (GA_ERR_STATE); a
 * null pointer anywhere (the message names the index), n_constraints above the cardinality or an nb_public the key contradicts is
 * GA_ERR_INVALID, decided before any device work.  On an error the contents of proofs_out are unspecified; the context and the key
 * stay usable.  count = 0 is GA_OK and touches nothing. */
int ga_g16_prove_batch(ga_g16_pk* pk, uint32_t count, const void* const* w, const void* const* a, const void* const* b,
                       const void* const* c, uint64_t n_constraints, uint64_t nb_public, const void* r, const void* s,
                       void* proofs_out);

/* Multi-GPU proving with a key sharded by base-point range (one context + one shard per GPU, every rank gets the whole
 * solution): ga_g16_prove_partial runs computeH and the five MSMs over this shard and returns the sums BEFORE
 * randomisation as Jacobian points  A | B1 | K+Z (G1Jac each) | B2 (G2Jac);  the caller all-gathers them (RCCL), adds them
 * with ga_jac_add and calls ga_g16_finish on the totals with (r, s).  ga_g16_prove == partial + finish on an unsharded key. */
int ga_g16_prove_partial(ga_g16_pk* pk, const void* w, const void* a, const void* b, const void* c,
                         uint64_t n_constraints, uint64_t nb_public, void* partials_out);
int ga_g16_finish(ga_g16_pk* pk, const void* partials_sum, const void* r, const void* s, void* proof_out);

/* The same proof in pieces, for callers that orchestrate several devices themselves (gnark_amd/multigpu.py does it with one
 * process per GPU and RCCL): the witness MSMs of this shard (A | B1 | K as G1Jac, B2 as G2Jac -- W is uploaded only over the wire
 * range the shard's bases cover), one chain of computeH per call (v = the solver's A, B or C on the host; out_dev = n fr elements
 * on this key's device, holding n * FFT_coset(iFFT(v)) afterwards -- the chain is UNSCALED: the 1/n of the inverse transform is
 * not applied here, ga_g16_h_combine divides by n^2 in its point-wise step; a chain buffer is therefore only meaningful as an input
 * of ga_g16_h_combine of the SAME library build, never as the coset evaluations themselves), the combination
 * h = iFFT_coset((a*b - c)/(g^n - 1)) in a_dev from three such chains
 * (bit-reversed), and the MSM of this shard's slice of pk.G1.Z with the matching slice of h (h_slice_dev points at element off_z).
 * ga_g16_shard_layout: out8 = {off_z, len_z, w_lo, w_hi, domain cardinality, nb_wires, window_shard_index, window_shard_count}
 * (a window-sharded key covers all of h and W: off_z = 0, len_z = n - 1).
 * ga_g16_table_layout: out2[0] = which vectors carry a window table -- bit 0 G1.A, 1 G1.B, 2 G1.Z, 3 G1.K, 4 G2.B (with precompute = 0
 * the library builds as many as fit the free HBM, in the order of preference A, B, K, Z, G2.B); out2[1] = which of those tables are
 * laid out by wire id and share the single witness sort (bit 0 A, 1 B, 3 K, 4 G2.B). */
int ga_g16_shard_layout(ga_g16_pk* pk, uint64_t* out8);
int ga_g16_table_layout(ga_g16_pk* pk, uint64_t* out2);
int ga_g16_witness_partial(ga_g16_pk* pk, const void* w, uint64_t nb_public, void* partials_out);
int ga_g16_h_chain(ga_g16_pk* pk, const void* v, uint64_t n_constraints, void* out_dev);
/* the same chain on a vector that already sits on the device (buf_dev: n fr elements of room, the first n_constraints hold the
 * solver's vector): for callers that bring A, B, C to the chain's device in pieces -- every GPU of a node uploading 1/N of each
 * vector over its own PCIe link and handing it on over xGMI (gnark_amd/multigpu.py) -- instead of one 512 MiB upload per chain */
int ga_g16_h_chain_dev(ga_g16_pk* pk, void* buf_dev, uint64_t n_constraints);
int ga_g16_h_combine(ga_g16_pk* pk, void* a_dev, const void* b_dev, const void* c_dev);
int ga_g16_z_partial(ga_g16_pk* pk, const void* h_slice_dev, void* partial_out);
/* One proof over the GPUs of a node from ONE process (what a Go caller uses: mi355x.WithDevices): keys[i] = shard i of n of the
 * same proving key, each created in its own context on its own device.  One host thread per device inside the call; computeH's
 * three chains run on the first three devices, their results and the slices of h move over xGMI (hipMemcpyPeerAsync); the
 * partial sums are added on the host and finished with (r, s).  Arguments as ga_g16_prove. */
int ga_g16_prove_multi(ga_g16_pk* const* keys, uint32_t n, const void* w, const void* a, const void* b, const void* c,
                       uint64_t n_constraints, uint64_t nb_public, const void* r, const void* s, void* proof_out);

/* ---- proving-key files -----------------------------------------------------------------------
 * replaces: ProvingKey.ReadFrom / UnsafeReadFrom (marshal.go:305-373: compressed or uncompressed points, told apart by their
 * flag bits) and ReadDump (marshal.go:449-539: raw memory images), read straight into HBM: the file streams through pinned
 * staging buffers, points are decoded (big-endian -> Montgomery, on-curve check, square roots of compressed points) by a device
 * kernel, and the dump's slices are copied without any arithmetic.  The format is recognised from the stream (the 0xdeadbeef
 * marker of WriteDump).  ga_g16_pk_read_mem / _fd do not check subgroup membership, and take a dump's points as they are
 * (UnsafeReadFrom semantics).  The _checked forms are ProvingKey.ReadFrom (the default decoder, marshal.go:305-312): same
 * parameters, and every point the read keeps -- this shard's slice of the five vectors, the five header points, the commitment
 * bases -- goes through the tests of ga_check_points where it first sits on the device, a dump's raw images included.  The first
 * bad point ends the read with GA_ERR_INVALID; ga_last_error names the vector, the index within the file's vector and which of
 * the two failures it was; nothing stays pinned and the context stays usable.  A shard checks what it keeps: the union of all
 * shards' checks covers the file.
 *   k_remove: the toRemove wire list of prove.go:231-235 -- it comes from the constraint system, not from the key file; NULL / 0
 *   for circuits without commitments.  precompute, shard_index, shard_count: as in ga_g16_key.
 * ga_g16_key_write_fd writes the host description of a key in the WriteTo (GA_KEY_FORMAT_COMPRESSED), WriteRawTo (RAW) or
 * WriteDump (DUMP) layout (marshal.go:231-300,378-445); points are encoded on the device. */
#define GA_KEY_FORMAT_COMPRESSED 0
#define GA_KEY_FORMAT_RAW 1
#define GA_KEY_FORMAT_DUMP 2
int ga_g16_pk_read_mem(ga_ctx* ctx, int curve, const uint8_t* data, size_t len, int32_t precompute, uint32_t shard_index,
                       uint32_t shard_count, const uint64_t* k_remove, uint64_t len_k_remove, ga_g16_pk** out, uint64_t* bytes_read);
int ga_g16_pk_read_fd(ga_ctx* ctx, int curve, int fd, int32_t precompute, uint32_t shard_index, uint32_t shard_count,
                      const uint64_t* k_remove, uint64_t len_k_remove, ga_g16_pk** out, uint64_t* bytes_read);
int ga_g16_pk_read_mem_checked(ga_ctx* ctx, int curve, const uint8_t* data, size_t len, int32_t precompute, uint32_t shard_index,
                               uint32_t shard_count, const uint64_t* k_remove, uint64_t len_k_remove, ga_g16_pk** out, uint64_t* bytes_read);
int ga_g16_pk_read_fd_checked(ga_ctx* ctx, int curve, int fd, int32_t precompute, uint32_t shard_index, uint32_t shard_count,
                              const uint64_t* k_remove, uint64_t len_k_remove, ga_g16_pk** out, uint64_t* bytes_read);
int ga_g16_key_write_fd(ga_ctx* ctx, const ga_g16_key* key, int format, int fd, uint64_t* bytes_written);
/* Proof.ReadFrom (marshal.go:62-86): Ar | Bs | Krs | u32 n | n commitments | CommitmentPok, compressed (WriteTo) or uncompressed
 * (WriteRawTo) points.  proof_out: Ar | Bs | Krs affine (Montgomery), commitments_out: room for max_commitments G1Affine. */
int ga_g16_proof_unmarshal(int curve, const uint8_t* data, size_t len, void* proof_out, void* commitments_out,
                           uint32_t max_commitments, uint32_t* n_commitments, void* pok_out, size_t* consumed);
/* one G1Affine / G2Affine from its wire encoding (curve.Decoder for a single point; host arithmetic)
 * What the decoder accepts -- here, in ga_g16_proof_unmarshal and in the key readers above, one rule:
 *   - flag bits: BN254 00 raw, 01 infinity, 10 / 11 compressed with the smaller / larger y; BLS12-381 bit 7 compressed, bit 6 infinity,
 *     bit 5 larger y, and 0b001, 0b011, 0b111 are malformed;
 *   - every coordinate below p (in G2 A1 and A0 each); compressed: x^3 + b is a square, the flag picks the root ("larger" in Fp2: by A1,
 *     by A0 only when A1 = 0); raw: y^2 = x^3 + b (stricter than an unchecked gnark read);
 *   - infinity is its flag and nothing else: every other bit of the encoding is zero over the bytes consumed (an infinity flag followed by
 *     anything else is GA_ERR_INVALID, as gnark-crypto's ErrInvalidInfinityEncoding); an all-zero raw point is infinity as well;
 *   - a single point and a point of a proof take their length from their own flag (a BN254 infinity, whose flag is the same in both
 *     modes, takes the mode of the proof's first finite point, compressed while none was seen); inside a key's vector the stream fixes
 *     mode and stride, and a point or an infinity carrying the other mode's flag (BLS12-381: 0x40 compressed, 0xC0 raw) is refused.
 * On GA_ERR_INVALID *consumed (and *n_commitments) are not written. */
int ga_point_unmarshal(int curve, int group, const uint8_t* data, size_t len, void* affine_out, size_t* consumed);

/* Proof.WriteTo wire format (marshal.go:33-58, no commitments): compressed Ar | Bs | Krs | u32 0 | PoK(inf).
 * Returns the number of bytes written in *len (164 for BN254, 244 for BLS12-381). */
int ga_g16_proof_marshal(int curve, const void* proof, uint8_t* out, size_t cap, size_t* len);

/* ---- BSB22 commitments ------------------------------------------------------------------
 * replaces: the two commitment MSM blocks of the ICICLE prover -- pk.CommitmentKeys[i].Commit inside the solver hint
 * (prove.go:84, icicle.go:834-873) and ProveKnowledge after the solve (prove.go:112-117, icicle.go:904-944).
 * values = privateCommittedValues[i] (host, fr Montgomery, ck_len[i] elements).  Both MSMs run on the pinned bases with one
 * upload of the scalars; outputs are G1Affine (Montgomery): the commitment the hint hashes, and this commitment's proof of
 * knowledge (kept by the caller until all commitments are done, then folded). */
int ga_g16_commit(ga_g16_pk* pk, uint32_t index, const void* values, uint64_t n_values, void* commitment_out, void* pok_out);
/* proof.CommitmentPok.Fold(poks, challenge) (prove.go:127): sum_i challenge^i * poks[i]; host arithmetic (a handful of points).
 * poks: n G1Affine; challenge: fr Montgomery; out: G1Affine. */
int ga_g16_fold_pok(int curve, const void* poks, uint64_t n, const void* challenge, void* out);
/* fr.Hash(msg, dst, count) of gnark-crypto (field/hash ExpandMsgXmd with SHA-256, L = 16 + fr.Bytes = 48 bytes per element,
 * big-endian reduction mod r; same code shape as internal/smallfields/tinyfield/element.go:456-481): the commitment hint's
 * hash_to_field.New("bsb22-commitment") (prove.go:57-58,88-98) and the fold challenge fr.Hash(..., "G16-BSB22", 1) (:123).
 * out: count fr elements, Montgomery.  Host only. */
int ga_hash_to_field(int curve, const uint8_t* msg, size_t msg_len, const uint8_t* dst, size_t dst_len, uint32_t count, void* out);
/* expand_message_xmd (RFC 9380 5.3.1, SHA-256) on its own, so that tests can pin it to std/hash/expand/expand_test.go:52-140 */
int ga_expand_message_xmd(const uint8_t* msg, size_t msg_len, const uint8_t* dst, size_t dst_len, size_t n, uint8_t* out);
/* Proof.WriteTo with commitments (marshal.go:33-58): Ar | Bs | Krs | u32be n | n compressed commitments | compressed PoK.
 * commitments: n G1Affine (may be NULL when n = 0), pok: G1Affine or NULL (= infinity). */
int ga_g16_proof_marshal_bsb22(int curve, const void* proof, const void* commitments, uint32_t n, const void* pok,
                               uint8_t* out, size_t cap, size_t* len);
/* Proof.WriteRawTo (marshal.go:25-30): the same layout with uncompressed points (G1 x | y, G2 x.A1 | x.A0 | y.A1 | y.A0). */
int ga_g16_proof_marshal_raw(int curve, const void* proof, const void* commitments, uint32_t n, const void* pok,
                             uint8_t* out, size_t cap, size_t* len);
/* G1Affine.Marshal() (uncompressed big-endian x | y; what SerializeCommitment hashes, constraint/commitment.go:76-89,
 * prove.go:88).  out: 64 bytes (BN254) / 96 bytes (BLS12-381). */
int ga_g1_marshal_uncompressed(int curve, const void* affine, uint8_t* out, size_t cap, size_t* len);

/* ---- profiling hooks (ICICLE_STEP_PROFILE analogue, icicle.go:72-75) ------------------------------------
 * When enabled, every kernel stage is bracketed by hipEvents on the stream it is launched on; ga_profile_read
 * returns "name=ms;name=ms;..." for the stages recorded since the last ga_profile_reset. */
int ga_profile_enable(ga_ctx* ctx, int on);
int ga_profile_reset(ga_ctx* ctx);
int ga_profile_read(ga_ctx* ctx, char* buf, size_t cap);

/* ---- test / bench support: on-device synthetic key material with known discrete logs --------------------
 * out[i] = [k_i]G (affine, Montgomery) where k_i = xoshiro-derived 64-bit values expanded from `seed`;
 * the same k_i are written (as canonical fr elements, 4 limbs) to dlogs_out (device) so that a test can check
 * MSM(s, P) == [sum s_i k_i] G with a field dot product (SURVEY 8c "known discrete log").  */
int ga_gen_bases(ga_ctx* ctx, int curve, int group, uint64_t seed, size_t n, void* bases_dev, void* dlogs_dev);
/* elements [first, first + n) of the same sequence: a rank of a multi-GPU run generates only its shard of a synthetic key */
int ga_gen_bases_at(ga_ctx* ctx, int curve, int group, uint64_t seed, uint64_t first, size_t n, void* bases_dev, void* dlogs_dev);
/* out[i] = uniform fr element (Montgomery) from a counter-based generator keyed by seed (device) */
int ga_gen_scalars(ga_ctx* ctx, int curve, uint64_t seed, size_t n, void* scalars_dev);
/* dot = sum a_i * b_i over fr; a Montgomery, b canonical (the dlogs above); result canonical LE (32 bytes, host) */
int ga_fr_dot(ga_ctx* ctx, int curve, const void* a_dev, const void* b_dev, size_t n, void* out_host);
/* [k]G for the group generator, k canonical LE 32 bytes (host arithmetic) -> Jacobian */
int ga_generator_mul(int curve, int group, const void* k_canonical_le32, void* out_jac);

/* integer-multiplier / FMA issue-rate microbenchmarks (SURVEY 8d asks for the v_mad_u64_u32 rate);
 * writes "name=Gops;..." */
int ga_microbench(ga_ctx* ctx, char* buf, size_t cap);
/* the shader clock the device holds right now, in MHz: one wave on a stream of its own compares the shader cycle counter with the
 * constant-rate one for `micros` microseconds.  Takes no context lock -- call it from a second thread while the load of interest runs
 * (tools/clock_probe.py: the bucket kernels run below the clock short microbenchmarks see). */
int ga_clock_probe(ga_ctx* ctx, uint32_t micros, double* mhz_out);

#ifdef __cplusplus
}
#endif
#endif /* GNARK_AMD_H */

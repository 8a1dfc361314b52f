"""BLS12-377 (curve id 2), the G1 / Fr side, on the functional emulation: every call in scope against pyref on a pyref.Curve built
outside the oracle (tests/bls12_377_cases.py), the refusals of everything out of scope, and the arithmetic facts the kernels lean on
for this curve's two fields.  tests/test_bls12_377_gpu.py runs the same cases, and the larger sizes, on the device."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bls12_377_cases as cases  # noqa: E402
import bls12_377_params as Q  # noqa: E402
import lazy_bounds  # noqa: E402
import pyref  # noqa: E402

R = Q.R


# ---- the numbers ----------------------------------------------------------------------------------------------------------------------
def test_parameters():
    """p, r from the seed; the generator's order; 22 generates Fr*; BETA by its identity on the generator"""
    assert Q.verify()
    b = Q.beta()
    assert b != 1 and pow(b, 3, Q.P) == 1


def test_root_of_unity_order_and_generator():
    """omega from fr_root_of_unity(2^47) has order exactly 2^47, and 22^((r-1)/q) != 1 for every prime q of r - 1"""
    c = cases.CURVE
    w = c.fr_root_of_unity(1 << 47)
    assert pow(w, 1 << 47, R) == 1 and pow(w, 1 << 46, R) == R - 1
    m = R - 1
    for q in Q.FR_MINUS_ONE_PRIMES:
        assert m % q == 0 and pow(22, (R - 1) // q, R) != 1, q
        while m % q == 0:
            m //= q
    assert m == 1 and (R - 1) % (1 << 48) != 0
    # the product header carries the same root (Montgomery form)
    src = open(os.path.join(ROOT, "gnark_amd", "csrc", "constants.h")).read()
    blk = src[src.index("struct BLS12_377_Fr"):]
    words = [int(x, 16) for x in blk[blk.index("ROOT[8] = {") + 11:blk.index("}", blk.index("ROOT[8] = {"))].replace("u", "").split(", ")]
    assert sum(v << (32 * i) for i, v in enumerate(words)) == (w << 256) % R
    assert "static constexpr int ADICITY = 47;" in blk and "G2X0" not in src[src.index("struct BLS12_377_Fp"):] and "FP2Z[" not in src[src.index("struct BLS12_377_Fp"):]


def test_generated_headers_are_current(tmp_path):
    """tools/gen_constants.py writes the two headers that are committed: the oracle's byte for byte (it knows two curves), the product's
    with the BLS12-377 blocks"""
    import gen_constants
    keep = {p: open(os.path.join(ROOT, p)).read() for p in ("gnark_amd/csrc/constants.h", "oracle/oracle_constants.h")}
    gen_constants.main(str(tmp_path / "constants.h"), str(tmp_path / "oracle_constants.h"))
    assert open(tmp_path / "constants.h").read() == keep["gnark_amd/csrc/constants.h"]
    assert open(tmp_path / "oracle_constants.h").read() == keep["oracle/oracle_constants.h"]


def test_lazy_bounds_g1():
    """every bound of the unreduced G1 formulas holds for the 377-bit p in BLS12-381's radix (14 x 28 bits) with the kernels' present
    subtraction constants, with the headroom asked of the other curves"""
    for fn in (lazy_bounds.check, lazy_bounds.check_add):
        out = fn("bls12-377", False)
        assert max(out["X"], out["Y"], out["P"], out["R"]) < out["limit"] - 2.5
    assert all(v < 392 - 2 for v in lazy_bounds.check_mdbl("bls12-377", False).values())
    for fn in (lazy_bounds.check_dbl, lazy_bounds.check_ladder):
        out = fn("bls12-377", False)
        assert all(v < out["limit"] - 2 for k, v in out.items() if k != "limit")


def test_plonk_constraint_kernel_takes_the_lazy_path():
    """the 253-bit Fr satisfies PLONK_LAZY (8 spare bits of the 9 x 29-bit limbs) and the bounds of plonk_constraints29_at with the
    maximum of 16 BSB22 gates: about 24 r of the 438 r that fit"""
    out = lazy_bounds.check_plonk_constraints(r=lazy_bounds.BLS12_377_R)
    assert out["res"] < 40 and out["limit"] > 400
    assert 9 * 29 - R.bit_length() >= 7 and 9 * 29 - 256 == 5


def test_barrett_step_on_the_two_fields():
    """f29_reduce_3p keeps 12 fraction bits of 2^(BITS+8) / p; for this curve's moduli the fraction lost is large (0.69 and 0.80), so
    the residue bound is not the 1.35 p of the other four fields.  Fr: below 3 r and 256 bits for ANY normalized value.  Fp: below
    3 p only for values below 2^386.5 -- the lazy G1 values stay below 2^380 (test_lazy_bounds_g1), where the residue is below 1.2 p"""
    p, L, NL, _ = lazy_bounds.CURVES["bls12-377"]
    worst, first_bad = lazy_bounds.check_reduce_3p(R, 29, 9)
    assert first_bad is None and worst < 1.9 and worst * R < 1 << 256
    worst, first_bad = lazy_bounds.check_reduce_3p(p, L, NL)
    assert first_bad is not None and first_bad > 386
    top = max(max(v for k, v in fn("bls12-377", False).items() if k != "limit")
              for fn in (lazy_bounds.check, lazy_bounds.check_add, lazy_bounds.check_dbl, lazy_bounds.check_ladder, lazy_bounds.check_mdbl))
    assert top < 380
    worst, first_bad = lazy_bounds.check_reduce_3p(p, L, NL, below_log2=top + 1)
    assert first_bad is None and worst < 1.2


def test_canonical_scalar_reduction_steps():
    """a canonical scalar may be any 256-bit integer: 2^256 / r - 1 conditional subtractions bring it below r -- 13 for this r, where
    the other two scalar fields need 5 and 2 (field.hip.h canonical_steps gives 16 and 6)"""
    assert ((1 << 256) - 1) // R == 13
    src = open(os.path.join(ROOT, "gnark_amd", "csrc", "field.hip.h")).read()
    assert "P::BITS + 2 >= 32 * P::N ? 6 : (1 << (32 * P::N - P::BITS + 1))" in src and 1 << (256 - 253 + 1) >= 13


def test_python_layer():
    from gnark_amd import _lib, device
    assert _lib.BLS12_377 == 2 and device.FP_LIMBS[2] == 6
    assert device.curve_id("bls12-377") == device.curve_id("bls12_377") == device.curve_id(2) == 2
    with pytest.raises(ValueError, match="bls12-377"):
        device.curve_id("bw6-761")


# ---- the calls, on the emulation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 1 << 8])
def test_msm(emu_ctx, n):
    cases.case_msm(emu_ctx, n)


@pytest.mark.parametrize("table_c", [11, 23])
def test_msm_table_width_dividing_253(emu_ctx, monkeypatch, table_c):
    """no n <= 2^8 is planned with c = 11; the table planner's knob forces it, and 23, the other divisor of 253"""
    cases.case_msm_table_width(emu_ctx, 1 << 8, table_c, monkeypatch)


def test_msm_plan_c11_range(emu_lib):
    """ga_msm_plan answers c = 11 on one run of sizes, 11265 .. 20479: its first size and 2^14 run on the device
    (tests/test_bls12_377_gpu.py); a size of that run costs the emulation a minute"""
    assert cases.plan_c11_sizes(emu_lib, 1 << 14) == [(11265, 1 << 14)]


def test_group_helpers_and_synthetic_inputs(emu_ctx):
    cases.case_group_helpers(emu_ctx.lib)
    cases.case_synthetic(emu_ctx)


@pytest.mark.parametrize("n", [2, 8, 1 << 10])
def test_fft(emu_ctx, n):
    cases.case_fft(emu_ctx, n)


def test_fft_batch(emu_ctx):
    cases.case_fft_batch(emu_ctx)


def test_compute_h(emu_ctx):
    cases.case_compute_h(emu_ctx)


@pytest.mark.parametrize("nb_bsb", [0, 1])
@pytest.mark.parametrize("n", [16, 1 << 8])
def test_plonk_grand_product_and_quotient(emu_ctx, n, nb_bsb):
    cases.case_plonk(emu_ctx, n, nb_bsb)


def test_plonk_batches(emu_ctx, monkeypatch):
    cases.case_plonk_batches(emu_ctx, monkeypatch)


def test_kzg_open(emu_ctx):
    cases.case_kzg_open(emu_ctx)


def test_fr_vectors_and_hash(emu_ctx):
    cases.case_fr_vectors(emu_ctx)


def test_batch_scalar_mul(emu_ctx):
    cases.case_batch_scalar_mul(emu_ctx)


@pytest.mark.parametrize("n", [1 << 4, 1 << 8])
def test_to_lagrange_g1(emu_ctx, n):
    cases.case_to_lagrange(emu_ctx, n)


def test_check_points(emu_ctx, monkeypatch):
    cases.case_check_points(emu_ctx, monkeypatch)


def test_refusals(emu_ctx):
    cases.case_refusals(emu_ctx)

"""The MSM fallback paths on the functional emulation: the cases of tests/msm_path_cases.py for the five MSM objects, at the sizes of the
device run (tests/test_msm_paths_gpu.py) except where a comment below says otherwise.  Which lines they enter is measured by tools/emu_coverage.sh (profiles/emu_coverage.txt)."""
import pytest

import msm_path_cases as cases

OBJ = pytest.mark.parametrize("c,group", cases.OBJECTS, ids=cases.OBJECT_IDS)


@OBJ
@pytest.mark.parametrize("cancel", [False, True], ids=["equal", "opposite"])
@pytest.mark.parametrize("n", [600, 17000])
def test_hot_bucket_of_equal_partials(emu_ctx, monkeypatch, c, group, n, cancel):
    # (the table run of the larger size for BN254 G1 alone: for the other objects the emulation spends 10 .. 40 s building the table)
    cases.case_hot_bucket(emu_ctx, c, group, n, monkeypatch, cancel=cancel, table=n < 1000 or (c.name, group) == ("bn254", 0))


@OBJ
@pytest.mark.parametrize("every_second", [False, True], ids=["every-bucket", "every-second-bucket"])
def test_equal_running_sums_in_lazy_reduction(emu_ctx, monkeypatch, c, group, every_second):
    cases.case_equal_running_sums(emu_ctx, c, group, 10, monkeypatch, every_second=every_second)


@OBJ
def test_two_level_exact_reduction(emu_ctx, monkeypatch, c, group):
    cases.case_two_level_exact(emu_ctx, c, group, monkeypatch)


# (every group size for BN254 G1; BLS12-381 G2, whose bucket sets of 2^19 .. 2^21 take the emulation ~10 s each, and BLS12-377 G1 with 2 and 4 here
# and with all six on the device)
@pytest.mark.parametrize("c,group,group_size", [cases.OBJECTS[0] + (m,) for m in (2, 4, 8, 16, 32, 64)] + [cases.OBJECTS[3] + (m,) for m in (2, 4)] + [cases.OBJECTS[4] + (m,) for m in (2, 4)],
                         ids=lambda v: getattr(v, "name", v))
def test_running_sum_group_size(emu_ctx, monkeypatch, c, group, group_size):
    cases.case_group_size(emu_ctx, c, group, group_size, monkeypatch)


@pytest.mark.parametrize("min_seg", [32, 64, 256])
def test_min_seg_on_hot_bucket(emu_ctx, monkeypatch, min_seg):
    cases.case_min_seg_hot_bucket(emu_ctx, min_seg, monkeypatch)
    cases.case_group_size(emu_ctx, cases.pyref.BN254, 0, 16, monkeypatch, min_seg=min_seg)   # 2^19 buckets: the task length IS min_seg


@OBJ
def test_exact_bucket_redo(emu_ctx, monkeypatch, c, group):
    cases.case_exact_bucket_redo(emu_ctx, c, group, monkeypatch)


# ---- the point-vector calls: branches the coverage report showed as never run for one object ------------------------------------------
def test_plain_ladder_with_infinities_and_zero_scalars_bls12_381_g2(emu_ctx, monkeypatch):
    cases.case_plain_ladder_with_skips(emu_ctx, cases.pyref.BLS12_381, 1, monkeypatch)


@pytest.mark.parametrize("c,T", [(cases.pyref.BLS12_381, (0, 2)), (cases.BLS12_377, (0, 1))], ids=["bls12-381", "bls12-377"])
def test_to_lagrange_inputs_summing_to_an_order_3_point(emu_ctx, c, T):
    cases.case_to_lagrange_small_order_sum(emu_ctx, c, T)


@pytest.mark.parametrize("uniform", ["0", "1"], ids=["consecutive-lanes", "uniform-scalar"])
def test_to_lagrange_bls12_377_seven_stages_both_lane_orders(emu_ctx, monkeypatch, uniform):
    import bls12_377_cases
    monkeypatch.setenv("GA_EC_NTT_UNIFORM", uniform)
    bls12_377_cases.case_to_lagrange(emu_ctx, 128)


def test_to_lagrange_bls12_377_equal_points(emu_ctx):
    cases.case_to_lagrange_equal_points(emu_ctx, cases.BLS12_377)


@pytest.mark.parametrize("c,group", cases.OBJECTS[:3], ids=cases.OBJECT_IDS[:3])
def test_plain_ladder_with_infinities_and_zero_scalars(emu_ctx, monkeypatch, c, group):
    cases.case_plain_ladder_with_skips(emu_ctx, c, group, monkeypatch)

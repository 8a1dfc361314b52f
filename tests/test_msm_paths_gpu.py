"""The MSM fallback paths on the device: the cases of tests/msm_path_cases.py at the sizes of the emulation run
(tests/test_msm_paths.py), plus what only the device reaches in seconds: the table run of the very hot bucket, the running-sum group
sizes 16, 32 and 64 (bucket sets of 2^19 .. 2^21) and the task-length knob where it decides the task length (from 2^19 buckets up)."""
import pytest

import msm_path_cases as cases

pytestmark = pytest.mark.gpu

OBJ = pytest.mark.parametrize("c,group", cases.OBJECTS, ids=cases.OBJECT_IDS)


@OBJ
@pytest.mark.parametrize("cancel", [False, True], ids=["equal", "opposite"])
@pytest.mark.parametrize("n", [600, 17000])
def test_hot_bucket_of_equal_partials(gpu_ctx, monkeypatch, c, group, n, cancel):
    cases.case_hot_bucket(gpu_ctx, c, group, n, monkeypatch, cancel=cancel)


@OBJ
@pytest.mark.parametrize("every_second", [False, True], ids=["every-bucket", "every-second-bucket"])
def test_equal_running_sums_in_lazy_reduction(gpu_ctx, monkeypatch, c, group, every_second):
    cases.case_equal_running_sums(gpu_ctx, c, group, 10, monkeypatch, every_second=every_second)


@OBJ
def test_two_level_exact_reduction(gpu_ctx, monkeypatch, c, group):
    cases.case_two_level_exact(gpu_ctx, c, group, monkeypatch)


@pytest.mark.parametrize("c,group", [cases.OBJECTS[i] for i in (0, 3, 4)], ids=[cases.OBJECT_IDS[i] for i in (0, 3, 4)])
@pytest.mark.parametrize("group_size", [2, 4, 8, 16, 32, 64])
def test_running_sum_group_size(gpu_ctx, monkeypatch, c, group, group_size):
    cases.case_group_size(gpu_ctx, c, group, group_size, monkeypatch)


@pytest.mark.parametrize("min_seg", [32, 64, 256])
def test_min_seg_on_hot_bucket(gpu_ctx, monkeypatch, min_seg):
    cases.case_min_seg_hot_bucket(gpu_ctx, min_seg, monkeypatch)
    cases.case_group_size(gpu_ctx, cases.pyref.BN254, 0, 16, monkeypatch, min_seg=min_seg)   # 2^19 buckets: the task length IS min_seg


@OBJ
def test_exact_bucket_redo(gpu_ctx, monkeypatch, c, group):
    cases.case_exact_bucket_redo(gpu_ctx, c, group, monkeypatch)


# ---- the point-vector calls: branches the coverage report showed as never run for one object ------------------------------------------
def test_plain_ladder_with_infinities_and_zero_scalars_bls12_381_g2(gpu_ctx, monkeypatch):
    cases.case_plain_ladder_with_skips(gpu_ctx, cases.pyref.BLS12_381, 1, monkeypatch)


@pytest.mark.parametrize("c,T", [(cases.pyref.BLS12_381, (0, 2)), (cases.BLS12_377, (0, 1))], ids=["bls12-381", "bls12-377"])
def test_to_lagrange_inputs_summing_to_an_order_3_point(gpu_ctx, c, T):
    cases.case_to_lagrange_small_order_sum(gpu_ctx, c, T)


@pytest.mark.parametrize("uniform", ["0", "1"], ids=["consecutive-lanes", "uniform-scalar"])
def test_to_lagrange_bls12_377_seven_stages_both_lane_orders(gpu_ctx, monkeypatch, uniform):
    import bls12_377_cases
    monkeypatch.setenv("GA_EC_NTT_UNIFORM", uniform)
    bls12_377_cases.case_to_lagrange(gpu_ctx, 128)


def test_to_lagrange_bls12_377_equal_points(gpu_ctx):
    cases.case_to_lagrange_equal_points(gpu_ctx, cases.BLS12_377)


@pytest.mark.parametrize("c,group", cases.OBJECTS[:3], ids=cases.OBJECT_IDS[:3])
def test_plain_ladder_with_infinities_and_zero_scalars(gpu_ctx, monkeypatch, c, group):
    cases.case_plain_ladder_with_skips(gpu_ctx, c, group, monkeypatch)

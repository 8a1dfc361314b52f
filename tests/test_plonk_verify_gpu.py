"""plonk.Verify on the device: the cases of plonk_verify_cases.py on a real MI355X.  The proofs come from that module's Python prover,
made once per session and tiled."""
import pytest

import plonk_verify_cases as pc

pytestmark = pytest.mark.gpu
CURVE_IDS = [c.name for c in pc.CURVES]


@pytest.mark.parametrize("nb_bsb", [0, 1, 2])
@pytest.mark.parametrize("n", [8, 64])
@pytest.mark.parametrize("c", pc.CURVES, ids=CURVE_IDS)
def test_rows_match_the_model_bit_for_bit(gpu_ctx, c, n, nb_bsb):
    pc.case_rows(gpu_ctx, c, n, nb_bsb)


@pytest.mark.parametrize("c", pc.CURVES, ids=CURVE_IDS)
def test_rows_at_edge_challenges(gpu_ctx, c):
    pc.case_edges(gpu_ctx, c)


@pytest.mark.parametrize("nb_public", [0, 3])
@pytest.mark.parametrize("nb_bsb", [0, 1, 2])
@pytest.mark.parametrize("n", [4, 16])
@pytest.mark.parametrize("cname", CURVE_IDS)
def test_proofs_of_the_python_prover_are_accepted(gpu_ctx, cname, n, nb_bsb, nb_public):
    if nb_public + nb_bsb > n:
        with pytest.raises(Exception, match="nb_public"):
            pc.blank_key(pc.pyref.CURVES[cname], n, nb_bsb, nb_public).device(gpu_ctx)
        return
    pc.case_acceptance(gpu_ctx, cname, n, nb_bsb, nb_public)


@pytest.mark.parametrize("cname", CURVE_IDS)
def test_a_proof_assembled_from_the_device_calls_is_accepted(gpu_ctx, cname):
    pc.case_device_loop(gpu_ctx, cname)


@pytest.mark.parametrize("cname", CURVE_IDS)
def test_every_tampered_field_is_rejected(gpu_ctx, cname):
    pc.case_tamper(gpu_ctx, cname, full_model=False)


@pytest.mark.parametrize("cname", CURVE_IDS)
def test_verify_many_gives_exact_verdicts(gpu_ctx, cname):
    pc.case_verify_many(gpu_ctx, cname, 1000)


@pytest.mark.parametrize("cname", CURVE_IDS)
def test_batch_verify_is_the_weighted_combination(gpu_ctx, cname):
    pc.case_batch(gpu_ctx, cname)


@pytest.mark.parametrize("cname", CURVE_IDS)
def test_a_bad_point_rejects_its_own_proof_only(gpu_ctx, cname):
    pc.case_point_checks(gpu_ctx, cname)


@pytest.mark.parametrize("c", pc.CURVES, ids=CURVE_IDS)
def test_errors_leave_the_context_usable(gpu_ctx, c):
    pc.case_errors(gpu_ctx, c)


@pytest.mark.parametrize("c", pc.CURVES, ids=CURVE_IDS)
def test_golden_key_files_decode_to_the_last_byte(gpu_ctx, c):
    pc.case_key_files(gpu_ctx, c)

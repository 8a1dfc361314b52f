"""plonk.Verify on the device, on the emulation build: ga_plonk_verify_scalars bit for bit against the model of plonk_verify_cases.py,
and Verify / VerifyMany / BatchVerify on proofs of that module's prover (whose SHA-256 transcript is its own, not gnark's)."""
import pytest

import plonk_verify_cases as pc

CURVE_IDS = [c.name for c in pc.CURVES]


@pytest.mark.parametrize("nb_bsb", [0, 1, 2])
@pytest.mark.parametrize("n", [8, 64])
@pytest.mark.parametrize("c", pc.CURVES, ids=CURVE_IDS)
def test_rows_match_the_model_bit_for_bit(emu_ctx, c, n, nb_bsb):
    pc.case_rows(emu_ctx, c, n, nb_bsb)


@pytest.mark.parametrize("c", pc.CURVES, ids=CURVE_IDS)
def test_rows_at_edge_challenges(emu_ctx, c):
    pc.case_edges(emu_ctx, c)


@pytest.mark.parametrize("nb_public", [0, 3])
@pytest.mark.parametrize("nb_bsb", [0, 1, 2])
@pytest.mark.parametrize("n", [4, 16])
@pytest.mark.parametrize("cname", CURVE_IDS)
def test_proofs_of_the_python_prover_are_accepted(emu_ctx, cname, n, nb_bsb, nb_public):
    if nb_public + nb_bsb > n:
        # n = 4 cannot hold three public inputs and two commitment rows: the key itself is refused (nb_public + nb_bsb above n)
        with pytest.raises(Exception, match="nb_public"):
            pc.blank_key(pc.pyref.CURVES[cname], n, nb_bsb, nb_public).device(emu_ctx)
        return
    pc.case_acceptance(emu_ctx, cname, n, nb_bsb, nb_public)


@pytest.mark.parametrize("cname", CURVE_IDS)
def test_a_proof_assembled_from_the_device_calls_is_accepted(emu_ctx, cname):
    pc.case_device_loop(emu_ctx, cname)


@pytest.mark.parametrize("cname", CURVE_IDS)
def test_every_tampered_field_is_rejected(emu_ctx, cname):
    pc.case_tamper(emu_ctx, cname, full_model=True)


@pytest.mark.parametrize("cname", CURVE_IDS)
def test_verify_many_gives_exact_verdicts(emu_ctx, cname):
    pc.case_verify_many(emu_ctx, cname, 37)


@pytest.mark.parametrize("cname", CURVE_IDS)
def test_batch_verify_is_the_weighted_combination(emu_ctx, cname):
    pc.case_batch(emu_ctx, cname)


@pytest.mark.parametrize("cname", CURVE_IDS)
def test_a_bad_point_rejects_its_own_proof_only(emu_ctx, cname):
    pc.case_point_checks(emu_ctx, cname)


@pytest.mark.parametrize("c", pc.CURVES, ids=CURVE_IDS)
def test_errors_leave_the_context_usable(emu_ctx, c):
    pc.case_errors(emu_ctx, c)


@pytest.mark.parametrize("c", pc.CURVES, ids=CURVE_IDS)
def test_golden_key_files_decode_to_the_last_byte(emu_ctx, c):
    pc.case_key_files(emu_ctx, c)

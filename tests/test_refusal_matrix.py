"""Unknown curve and group ids at every entry point of the C ABI that takes a curve (tests/refusal_matrix_cases.py), on the functional
emulation and on the device.  Nothing is launched: every call is refused at its entry."""
import pytest

import refusal_matrix_cases as cases


def test_table_has_every_entry_point_with_a_curve_parameter():
    cases.check_table_complete()


def test_refusal_matrix(emu_ctx):
    cases.case_refusal_matrix(emu_ctx)


@pytest.mark.gpu
def test_refusal_matrix_on_the_device(gpu_ctx):
    cases.case_refusal_matrix(gpu_ctx)

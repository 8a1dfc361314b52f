"""The refusal matrix of the C ABI: what every entry point with a curve parameter answers to a curve or group id that does not exist.
tests/test_refusal_matrix.py runs it on the functional emulation and on the device; no call here gets as far as a launch.

ROWS has one raw ctypes call per entry point of include/gnark_amd.h with an `int curve` parameter, on BN254-shaped operands of four
elements (check_table_complete: a new entry point cannot stay out of it).  What curve id 2 is answered where it is not built is
tests/bls12_377_cases.py::case_refusals' subject, not this table's."""
import ctypes as C
import os
import re
import types

import numpy as np

import pyref
from gnark_amd import _lib
from gnark_amd.device import _ptr
from helpers import fr_to_arr, g1_to_arr, g2_to_arr

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gnark_amd.h")
GA_ERR_INVALID = -1
UNKNOWN_CURVE, UNKNOWN_GROUP = 7, 5


def prototypes():
    """{entry point: [parameter names]} of include/gnark_amd.h (the functions test_abi_surface.declared_functions() finds)"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(ga_[a-z0-9_]+)\s*\(([^;{)]*)\)\s*;", src):
        out[name] = [re.findall(r"\w+", p)[-1] for p in params.split(",") if p.strip() and p.strip() != "void"]
    return out


def operands(ctx):
    bn = pyref.BN254
    o = types.SimpleNamespace(h=ctx.handle)
    o.g1, o.g2, o.fr = _ptr(g1_to_arr(bn, [bn.g1] * 4)), _ptr(g2_to_arr(bn, [bn.g2] * 4)), _ptr(fr_to_arr(bn, [1, 2, 3, 4]))
    o.jac = _ptr(np.zeros(2 * 24, dtype=np.uint64))                     # two Jacobian points of either group, (0, 0, 0)
    o.out = _ptr(np.zeros(256, dtype=np.uint64))
    o.rows = _ptr(np.arange(5, dtype=np.uint64))                        # four rows (or groups) of one term (or pair) each
    o.terms = _ptr(np.array([[i, i] for i in range(4)], dtype=np.uint32))
    o.bytes = _ptr(np.zeros(256, dtype=np.uint8))
    o.vecs = (C.c_void_p * 2)(o.fr, o.fr)
    o.fd = os.open(os.devnull, os.O_RDONLY)
    return o


def _i():
    return C.byref(C.c_int())


def _p():
    return C.byref(C.c_void_p())


def _z():
    return C.byref(C.c_size_t())


# entry point -> (the parameter that counts elements and may be 0, or None; arguments for (operands, curve, group, count))
ROWS = {
    "ga_msm": ("n", lambda o, cv, gp, n: [o.h, cv, gp, o.g1, o.fr, n, 0, o.out]),
    "ga_msm_windows": ("n", lambda o, cv, gp, n: [o.h, cv, gp, o.g1, o.fr, n, 0, 0, -1, o.out, _i(), _i()]),
    "ga_msm_plan": ("n", lambda o, cv, gp, n: [cv, gp, n, _i(), _i()]),
    "ga_msm_combine_windows": (None, lambda o, cv, gp, n: [cv, gp, o.jac, 2, 4, o.out]),
    "ga_batch_scalar_mul": ("n", lambda o, cv, gp, n: [o.h, cv, gp, o.g1, o.fr, n, 0, o.out]),
    "ga_batch_scalar_mul_plan": ("n", lambda o, cv, gp, n: [cv, n, _i(), _i()]),
    "ga_kzg_to_lagrange_g1": ("n", lambda o, cv, gp, n: [o.h, cv, o.g1, n, 0, o.out]),
    "ga_lagrange_coeffs": ("n", lambda o, cv, gp, n: [o.h, cv, gp, o.g1, n, 0, o.out]),
    "ga_scale_points": ("n", lambda o, cv, gp, n: [o.h, cv, gp, o.g1, n, 0, o.fr, 0, 0, o.out, None]),
    "ga_check_points": ("n", lambda o, cv, gp, n: [o.h, cv, gp, o.g1, n, 0, o.bytes, (C.c_uint64 * 4)()]),
    "ga_pairing_check": ("n_groups", lambda o, cv, gp, n: [o.h, cv, o.g1, o.g2, 4, o.rows, n, 0, o.bytes, None, (C.c_uint64 * 2)()]),
    "ga_sparse_point_sums": ("n_rows", lambda o, cv, gp, n: [o.h, cv, gp, o.g1, 4, o.rows, n, o.terms, o.fr, 4, 0, o.out, None]),
    "ga_fr_lagrange_at": ("m", lambda o, cv, gp, n: [o.h, cv, 4, o.fr, n, 0, o.out]),
    "ga_fr_sparse_matvec": ("n_rows", lambda o, cv, gp, n: [o.h, cv, o.fr, 4, o.rows, n, o.terms, o.fr, 4, None, None, 0, 0, o.out]),
    "ga_fr_compact_nonzero": ("n", lambda o, cv, gp, n: [o.h, cv, o.fr, n, 0, o.out, None, C.byref(C.c_uint64())]),
    "ga_fr_powers": ("n", lambda o, cv, gp, n: [o.h, cv, o.fr, 0, n, 0, o.out]),
    "ga_msm_table_create": (None, lambda o, cv, gp, n: [o.h, cv, gp, o.g1, 4, 0, _p()]),
    "ga_jac_add": (None, lambda o, cv, gp, n: [cv, gp, o.jac, o.jac, o.out]),
    "ga_jac_to_affine": (None, lambda o, cv, gp, n: [cv, gp, o.jac, o.out]),
    "ga_jac_scalar_mul": (None, lambda o, cv, gp, n: [cv, gp, o.jac, o.fr, o.out]),
    "ga_domain_create": (None, lambda o, cv, gp, n: [o.h, cv, 4, _p()]),
    "ga_fr_linear_combination": ("n", lambda o, cv, gp, n: [o.h, cv, n, 2, o.vecs, o.fr, o.out, 0]),
    "ga_fr_poly_evaluate": ("n", lambda o, cv, gp, n: [o.h, cv, o.fr, n, o.fr, o.out, 0]),
    "ga_fr_vec_mul": ("n", lambda o, cv, gp, n: [o.h, cv, o.fr, o.fr, n, o.out, 0]),
    "ga_fr_batch_invert": ("n", lambda o, cv, gp, n: [o.h, cv, o.out, n, 0]),
    "ga_g16_builder_create": (None, lambda o, cv, gp, n: [o.h, cv, 4, 3, 0, 1, _p()]),
    "ga_g16_pk_read_mem": (None, lambda o, cv, gp, n: [o.h, cv, o.bytes, 256, -1, 0, 1, None, 0, _p(), None]),
    "ga_g16_pk_read_fd": (None, lambda o, cv, gp, n: [o.h, cv, o.fd, -1, 0, 1, None, 0, _p(), None]),
    "ga_g16_pk_read_mem_checked": (None, lambda o, cv, gp, n: [o.h, cv, o.bytes, 256, -1, 0, 1, None, 0, _p(), None]),
    "ga_g16_pk_read_fd_checked": (None, lambda o, cv, gp, n: [o.h, cv, o.fd, -1, 0, 1, None, 0, _p(), None]),
    "ga_g16_proof_unmarshal": (None, lambda o, cv, gp, n: [cv, o.bytes, 256, o.out, None, 0, None, None, None]),
    "ga_point_unmarshal": (None, lambda o, cv, gp, n: [cv, gp, o.bytes, 256, o.out, None]),
    "ga_g16_proof_marshal": (None, lambda o, cv, gp, n: [cv, o.jac, o.out, 2048, _z()]),
    "ga_g16_fold_pok": ("n", lambda o, cv, gp, n: [cv, o.g1, n, o.fr, o.out]),
    "ga_hash_to_field": ("count", lambda o, cv, gp, n: [cv, o.bytes, 3, o.bytes, 3, n, o.out]),
    "ga_g16_proof_marshal_bsb22": ("n", lambda o, cv, gp, n: [cv, o.jac, o.g1, n, o.g1, o.out, 2048, _z()]),
    "ga_g16_proof_marshal_raw": ("n", lambda o, cv, gp, n: [cv, o.jac, o.g1, n, o.g1, o.out, 2048, _z()]),
    "ga_g1_marshal_uncompressed": (None, lambda o, cv, gp, n: [cv, o.g1, o.out, 2048, _z()]),
    "ga_gen_bases": ("n", lambda o, cv, gp, n: [o.h, cv, gp, 3, n, o.out, None]),
    "ga_gen_bases_at": ("n", lambda o, cv, gp, n: [o.h, cv, gp, 3, 0, n, o.out, None]),
    "ga_gen_scalars": ("n", lambda o, cv, gp, n: [o.h, cv, 3, n, o.out]),
    "ga_fr_dot": ("n", lambda o, cv, gp, n: [o.h, cv, o.fr, o.fr, n, o.out]),
    "ga_generator_mul": (None, lambda o, cv, gp, n: [cv, gp, o.fr, o.out]),
}


def check_table_complete():
    protos = prototypes()
    with_curve = sorted(f for f, params in protos.items() if "curve" in params)
    assert len(with_curve) > 40 and with_curve == sorted(ROWS), set(with_curve) ^ set(ROWS)
    for f, (count, _) in ROWS.items():
        assert count is None or count in protos[f], (f, count)


def _refused(lib, name, rc, what):
    msg = lib.ga_last_error().decode()
    assert rc == GA_ERR_INVALID, (name, what, rc, msg)
    assert what in msg and name in msg, (name, what, msg)


def case_refusal_matrix(ctx):
    """curve id 7 -- with four elements, and with none where the call has a count: the check comes before the n = 0 shortcut -- and
    group ids 5 and -1 on BN254: GA_ERR_INVALID and a message that names the id and the entry point; the context then takes a BN254 call"""
    lib, o, protos = ctx.lib, operands(ctx), prototypes()
    try:
        for name, (count, args) in ROWS.items():
            fn = getattr(lib, name)
            tries = [(UNKNOWN_CURVE, 0, 4, "unknown curve id %d" % UNKNOWN_CURVE)]
            if count:
                tries.append((UNKNOWN_CURVE, 0, 0, "unknown curve id %d" % UNKNOWN_CURVE))
            if "group" in protos[name]:
                tries.append((0, UNKNOWN_GROUP, 4, "unknown group id %d" % UNKNOWN_GROUP))
                tries.append((0, -1, 4, "unknown group id -1"))
                tries.append((UNKNOWN_CURVE, UNKNOWN_GROUP, 4, "unknown curve id %d" % UNKNOWN_CURVE))   # both unknown: the curve is reported
            for cv, gp, n, what in tries:
                _refused(lib, name, fn(*args(o, cv, gp, n)), what)
                # the refusal left no lock behind: an empty BN254 call that takes the context, and one without a context
                assert lib.ga_fr_vec_mul(o.h, 0, o.fr, o.fr, 0, o.out, 0) == _lib.GA_OK, (name, lib.ga_last_error().decode())
                assert lib.ga_msm_plan(0, 0, 4, _i(), _i()) == _lib.GA_OK, (name, lib.ga_last_error().decode())
    finally:
        os.close(o.fd)

"""The C ABI is compiled from several host units: the error buffer must still be ONE thread-local buffer for the
whole library -- a failure in any unit is what gp_last_error_string() reports -- and every message must have
survived the move.  No GPU: NULL handles make each entry fail in its own unit's argument checks."""
import ctypes
import threading

import pytest

from gp_emulator_amd import _lib

GP_ERR_INVALID = -1
i32, i64 = ctypes.c_int(), ctypes.c_int64()
ref = ctypes.byref

# (entry, arguments, message): one entry at least from every host unit
CASES = [
    ("gp_pack_model_f64", [None] * 4 + [3, 1, 3] + [None] * 4, "null pointer"),
    ("gp_launch_plan", [99, _lib.GP_F64, 10, 2, 1, 1, 0, 1, 0, ref(i32), ref(i64), ref(i32), ref(i64), ref(i32), ref(i32)],
     "bad op 99"),
    ("gp_predict_host", [None, None, _lib.GP_F64, None, None, None, None, 1, 0, 0], "null context or model"),
    ("gp_mv_predict_host", [None, None, None, None, 1, 1, None, None], "null context or model"),
    ("gp_hessian_weighted_host", [None, None, _lib.GP_F64, None, None, None, 1], "null context or model"),
    ("gp_band_misfit_host", [None, None, _lib.GP_F64, None, None, 1, 1, None, 1, 1, None, None, None, None, None, 1],
     "null context or model"),
    ("gp_reconstruct_device", [None, _lib.GP_F64, None, None, None, 1, 1, 1], "null context"),
    ("gp_mv_misfit_device", [None, _lib.GP_F64, None, None, None, None, 0, None, 0, None, None, None, 1, 1, 1, 1],
     "null context"),
    ("gp_likelihood_batch_f64", [None, 1, None, None, None, 1, 1, 1, None, None, None, None], "null context"),
    ("gp_malloc", [None, 16, None], "null pointer"),
    ("gp_event_create", [None, None], "null pointer"),
]


def fail_with(lib, name, args):
    rc = getattr(lib, name)(*args)
    return rc, lib.gp_last_error_string().decode()


@pytest.mark.parametrize("name,args,message", CASES, ids=[c[0] for c in CASES])
def test_every_unit_reports_through_the_one_error_buffer(name, args, message):
    lib = _lib.load()
    # a different message first, so that a unit writing to a buffer of its own would leave this one behind
    other = CASES[1] if message != CASES[1][2] else CASES[0]
    assert fail_with(lib, other[0], other[1]) == (GP_ERR_INVALID, other[2])
    assert fail_with(lib, name, args) == (GP_ERR_INVALID, message)


def test_error_buffer_is_per_thread():
    lib = _lib.load()
    assert fail_with(lib, *CASES[1][:2]) == (GP_ERR_INVALID, "bad op 99")
    seen = []
    t = threading.Thread(target=lambda: seen.append(fail_with(lib, *CASES[6][:2])))
    t.start()
    t.join()
    assert seen == [(GP_ERR_INVALID, "null context")]
    assert lib.gp_last_error_string().decode() == "bad op 99"

"""CPU-side checks of the device best-response ABI (include/rp_mi355x.h: rp_mccfr_exploitability_device, rp_mccfr_best_response,
rp_mccfr_nash_variant, rp_mccfr_solve_to): the symbols exist, and the arguments a call is refused for are refused before a device is
needed, with the argument's name in rp_last_error."""
import ctypes as C
import os

import pytest

from robopoker_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rp_mi355x.h")
SYMBOLS = ("rp_mccfr_exploitability_device", "rp_mccfr_best_response", "rp_mccfr_nash_variant", "rp_mccfr_solve_to")


def test_symbols_exist():
    lib = _lib.load()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.declared_symbols()
    text = open(HEADER).read()
    for name in SYMBOLS:
        assert f"RP_API int {name}(" in text


def test_null_arguments_are_invalid_and_named():
    lib = _lib.load()
    out = C.c_float()
    assert lib.rp_mccfr_exploitability_device(None, None) == _lib.RP_ERR_INVALID
    assert b"out_dev" in lib.rp_last_error()
    assert lib.rp_mccfr_exploitability_device(None, C.addressof(out)) == _lib.RP_ERR_INVALID
    assert b"h is NULL" in lib.rp_last_error()
    assert lib.rp_mccfr_best_response(None, None, None, None, None) == _lib.RP_ERR_INVALID
    assert b"h is NULL" in lib.rp_last_error()
    v = C.c_int()
    assert lib.rp_mccfr_nash_variant(None, C.byref(v)) == _lib.RP_ERR_INVALID
    assert b"h is NULL" in lib.rp_last_error()


@pytest.mark.parametrize("target,check_every,word", [(0.5, 0, b"check_every"), (float("nan"), 4, b"target"), (float("nan"), 0, b"check_every"),
                                                     (0.5, 4, b"h is NULL")])
def test_solve_to_refuses_before_a_device_is_needed(target, check_every, word):
    lib = _lib.load()
    steps, e, hit = C.c_uint64(), C.c_float(), C.c_int()
    assert lib.rp_mccfr_solve_to(None, target, check_every, 16, C.byref(steps), C.byref(e), C.byref(hit)) == _lib.RP_ERR_INVALID
    assert word in lib.rp_last_error()
    assert lib.rp_mccfr_solve_to(None, target, check_every, 16, None, None, None) == _lib.RP_ERR_INVALID

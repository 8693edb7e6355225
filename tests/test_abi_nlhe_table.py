"""CPU-side checks of the table calls of the NLHE trainer (include/rp_mi355x.h, THE TABLE ITSELF ON THE DEVICE): the five symbols exist
with the documented signatures in the header, the library and the ctypes binding, a NULL handle is refused by each before a device is
needed, and none of them is a diagnostics call."""
import ctypes as C
import os
import re

from robopoker_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rp_mi355x.h")
DIAG = os.path.join(ROOT, "include", "rp_mi355x_diag.h")
# the parameter types of each prototype, in order ("T*" for any pointer to T, const or not)
CALLS = {
    "rp_nlhe_capacity": ["rp_nlhe*", "uint32_t*", "uint64_t*"],
    "rp_nlhe_resize": ["rp_nlhe*", "uint32_t"],
    "rp_nlhe_set_growth": ["rp_nlhe*", "uint32_t", "uint64_t"],
    "rp_nlhe_export_device": ["rp_nlhe*", "uint64_t", "uint64_t*", "uint64_t*", "uint32_t*", "uint64_t*", "rp_encounter*"],
    "rp_nlhe_import_device": ["rp_nlhe*", "uint64_t", "uint64_t*", "uint32_t*", "uint64_t*", "rp_encounter*", "uint64_t"],
}
CTYPES = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64}


def _prototype(text, name):
    m = re.search(r"RP_API\s+int\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, name
    params = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    out = []
    for p in params:
        words = p.replace("const", " ").replace("*", " * ").split()
        out.append(words[0] + ("*" if "*" in words else ""))
    return out


def test_the_five_symbols_exist_with_the_documented_signatures():
    lib, text = _lib.load(), open(HEADER).read()
    for name, params in CALLS.items():
        assert _prototype(text, name) == params, name
        assert hasattr(lib, name) and name in _lib.declared_symbols(), name
        res, args = _lib._SIGNATURES[name]
        assert res is C.c_int and len(args) == len(params), name
        for a, p in zip(args, params):
            if p in CTYPES:  # a scalar travels by value with its own width
                assert a is CTYPES[p], (name, p)
            else:
                assert a is C.c_void_p or a is C.POINTER(CTYPES[p[:-1]]), (name, p)


def test_a_null_handle_is_invalid_before_any_device_work():
    lib = _lib.load()
    cap, keys, n = C.c_uint32(), C.c_uint64(), C.c_uint64()
    assert lib.rp_nlhe_capacity(None, C.byref(cap), C.byref(keys)) == _lib.RP_ERR_INVALID and b"rp_nlhe_capacity" in lib.rp_last_error()
    assert lib.rp_nlhe_resize(None, 12) == _lib.RP_ERR_INVALID and b"rp_nlhe_resize" in lib.rp_last_error()
    assert lib.rp_nlhe_set_growth(None, 20, 0) == _lib.RP_ERR_INVALID and b"rp_nlhe_set_growth" in lib.rp_last_error()
    assert lib.rp_nlhe_export_device(None, 0, C.byref(n), None, None, None, None) == _lib.RP_ERR_INVALID
    assert b"rp_nlhe_export_device" in lib.rp_last_error()
    assert lib.rp_nlhe_import_device(None, 0, None, None, None, None, 0) == _lib.RP_ERR_INVALID
    assert b"rp_nlhe_import_device" in lib.rp_last_error()


def test_the_table_calls_are_not_diagnostics():
    diag = open(DIAG).read()
    for name in CALLS:
        assert name not in diag, name

"""CPU-side checks of the depth-solver ABI (include/rp_mi355x.h, rp_nlhe_depth_solve): the symbols exist, the three structs have the sizes
the header states, and the arguments a call is refused for are refused before a device is needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from robopoker_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rp_mi355x.h")
STRUCTS = {"rp_nlhe_depth_args": _lib.NlheDepthArgs, "rp_nlhe_depth_result": _lib.NlheDepthResult, "rp_nlhe_depth_row": _lib.NlheDepthRow}


def test_symbols_exist():
    lib = _lib.load()
    for name in ("rp_nlhe_depth_args_default", "rp_nlhe_depth_solve", "rp_nlhe_depth_solve_device"):
        assert hasattr(lib, name) and name in _lib.declared_symbols()


def test_struct_sizes_are_the_headers(tmp_path):
    text = open(HEADER).read()
    stated = {}
    for name, mirror in STRUCTS.items():
        m = re.search(r"\}\s*%s;\s*/\*\s*(\d+) bytes\s*\*/" % name, text)
        assert m, f"{name}: the header states no size"
        stated[name] = int(m.group(1))
        assert C.sizeof(mirror) == stated[name], name
    # and a C compiler, where there is one, agrees with what the header states
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    if cc is not None:
        src = tmp_path / "sizes.c"
        src.write_text('#include "rp_mi355x.h"\n' + "".join(f'_Static_assert(sizeof({n}) == {b}, "{n}");\n' for n, b in stated.items()))
        subprocess.check_call([cc, "-std=c11", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)])


def test_defaults_are_the_references():
    a = _lib.NlheDepthArgs()
    _lib.load().rp_nlhe_depth_args_default(C.byref(a))
    # FrontierHyperParams::default (subgame/src/depth/hyperparams.rs), WarmstartHyperParams::default (mccfr/src/hyperparams/warmstart.rs)
    assert (a.iterations, a.rollouts, a.bias, a.prior, a.seed, a.first_id, a.rows_cap, a.reserved) == (1, 16, 5.0, 16384.0, 0, 0, 0, 0)


@pytest.mark.parametrize("field,value,word", [
    ("iterations", 0, b"iterations"), ("iterations", _lib.RP_NLHE_DEPTH_MAX_ITERATIONS + 1, b"iterations"), ("rollouts", 4097, b"rollouts"),
    ("bias", 0.0, b"bias"), ("bias", -1.0, b"bias"), ("bias", float("inf"), b"bias"), ("bias", float("nan"), b"bias"),
    ("prior", 0.0, b"prior"), ("prior", float("nan"), b"prior"), ("prior", float("inf"), b"prior"), ("reserved", 1, b"reserved")])
def test_bad_args_are_invalid(field, value, word):
    lib = _lib.load()
    a = _lib.NlheDepthArgs()
    lib.rp_nlhe_depth_args_default(C.byref(a))
    setattr(a, field, value)
    for fn in (lib.rp_nlhe_depth_solve, lib.rp_nlhe_depth_solve_device):
        for n in (0, 1):
            assert fn(None, n, None, None, C.byref(a), None, None) == _lib.RP_ERR_INVALID
            assert word in lib.rp_last_error()


def test_null_args_and_an_empty_batch():
    lib = _lib.load()
    a = _lib.NlheDepthArgs()
    lib.rp_nlhe_depth_args_default(C.byref(a))
    for fn in (lib.rp_nlhe_depth_solve, lib.rp_nlhe_depth_solve_device):
        assert fn(None, 0, None, None, None, None, None) == _lib.RP_ERR_INVALID
        assert fn(None, 0, None, None, C.byref(a), None, None) == _lib.RP_OK  # n = 0: no launch, nothing is looked at
        a.rollouts = 0  # reads as 1
        assert fn(None, 0, None, None, C.byref(a), None, None) == _lib.RP_OK
        assert fn(None, 1, None, None, C.byref(a), None, None) == _lib.RP_ERR_INVALID
        assert b"handle" in lib.rp_last_error()

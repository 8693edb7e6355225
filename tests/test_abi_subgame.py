"""CPU-side checks of the safe-subgame-solver ABI (include/rp_mi355x.h, rp_nlhe_subgame_solve): the symbols exist, the four structs have
the sizes the header states, and the arguments a call is refused for are refused before a device is needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from robopoker_amd import _lib, nlhe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rp_mi355x.h")
STRUCTS = {"rp_nlhe_subgame_args": _lib.NlheSubgameArgs, "rp_nlhe_subgame_result": _lib.NlheSubgameResult,
           "rp_nlhe_subgame_row": _lib.NlheSubgameRow, "rp_nlhe_subgame_deal": _lib.NlheSubgameDeal}
FORMS = ("rp_nlhe_subgame_solve", "rp_nlhe_subgame_solve_device")


def call(fn, n, args, h=None, entries=None, hole_world=None, weights=None, results=None, rows=None, deals=None):
    return fn(h, n, entries, hole_world, weights, None, args, results, rows, deals)


def defaults():
    a = _lib.NlheSubgameArgs()
    _lib.load().rp_nlhe_subgame_args_default(C.byref(a))
    return a


def test_symbols_exist():
    lib = _lib.load()
    for name in ("rp_nlhe_subgame_args_default",) + FORMS:
        assert hasattr(lib, name) and name in _lib.declared_symbols()


def test_struct_sizes_are_the_headers(tmp_path):
    text = open(HEADER).read()
    stated = {}
    for name, mirror in STRUCTS.items():
        m = re.search(r"\}\s*%s;\s*/\*\s*(\d+) bytes\s*\*/" % name, text)
        assert m, f"{name}: the header states no size"
        stated[name] = int(m.group(1))
        assert C.sizeof(mirror) == stated[name], name
    assert stated == {"rp_nlhe_subgame_args": 48, "rp_nlhe_subgame_result": 176, "rp_nlhe_subgame_row": 168, "rp_nlhe_subgame_deal": 16}
    assert (nlhe.SUBGAME_RESULT_DTYPE.itemsize, nlhe.SUBGAME_ROW_DTYPE.itemsize, nlhe.SUBGAME_DEAL_DTYPE.itemsize) == (176, 168, 16)
    # the result is the depth result with the deals' counters behind it; the numpy views agree with the ctypes mirrors field by field
    for dtype, mirror in ((nlhe.SUBGAME_RESULT_DTYPE, _lib.NlheSubgameResult), (nlhe.SUBGAME_ROW_DTYPE, _lib.NlheSubgameRow),
                          (nlhe.SUBGAME_DEAL_DTYPE, _lib.NlheSubgameDeal)):
        assert {f: dtype.fields[f][1] for f in dtype.names} == {f: getattr(mirror, f).offset for f, _ in mirror._fields_}
    assert all(getattr(_lib.NlheSubgameResult, f).offset == getattr(_lib.NlheDepthResult, f).offset for f, _ in _lib.NlheDepthResult._fields_)
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    if cc is not None:
        src = tmp_path / "sizes.c"
        src.write_text('#include "rp_mi355x.h"\n' + "".join(f'_Static_assert(sizeof({n}) == {b}, "{n}");\n' for n, b in stated.items()))
        subprocess.check_call([cc, "-std=c11", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)])


def test_constants_are_the_headers():
    text = open(HEADER).read()
    for name, value in (("RP_NLHE_SUBGAME_MAX_ROWS", _lib.RP_NLHE_SUBGAME_MAX_ROWS), ("RP_NLHE_SUBGAME_ORIGIN_NONE", _lib.RP_NLHE_SUBGAME_ORIGIN_NONE)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value
    assert _lib.RP_NLHE_SUBGAME_ORIGIN_NONE not in range(-1, 4) and _lib.RP_NLHE_SUBGAME_ORIGIN_NONE != _lib.RP_NLHE_DEPTH_ORIGIN_ENTRY


def test_defaults_are_the_references():
    a = defaults()
    assert (a.iterations, a.rollouts, a.bias, a.prior, a.seed, a.first_id, a.rows_cap, a.deals_cap, tuple(a.reserved)) == \
        (1, 16, 5.0, 16384.0, 0, 0, 0, 0, (0, 0))


@pytest.mark.parametrize("field,value,word", [
    ("iterations", 0, b"iterations"), ("iterations", _lib.RP_NLHE_DEPTH_MAX_ITERATIONS + 1, b"iterations"), ("rollouts", 4097, b"rollouts"),
    ("bias", 0.0, b"bias"), ("bias", -1.0, b"bias"), ("bias", float("inf"), b"bias"), ("bias", float("nan"), b"bias"),
    ("prior", 0.0, b"prior"), ("prior", -2.0, b"prior"), ("prior", float("nan"), b"prior"), ("prior", float("inf"), b"prior"),
    ("reserved", (1, 0), b"reserved"), ("reserved", (0, 1), b"reserved")])
def test_bad_args_are_invalid(field, value, word):
    lib = _lib.load()
    a = defaults()
    setattr(a, field, (C.c_uint32 * 2)(*value) if field == "reserved" else value)
    for name in FORMS:
        for n in (0, 1):
            assert call(getattr(lib, name), n, C.byref(a)) == _lib.RP_ERR_INVALID
            assert word in lib.rp_last_error()


def test_null_args_and_an_empty_batch():
    lib = _lib.load()
    for name in FORMS:
        fn, a = getattr(lib, name), defaults()
        assert call(fn, 0, None) == _lib.RP_ERR_INVALID
        assert call(fn, 0, C.byref(a)) == _lib.RP_OK  # n = 0: no launch, nothing is looked at
        a.rollouts = 0  # reads as 1
        assert call(fn, 0, C.byref(a)) == _lib.RP_OK
        a.iterations = _lib.RP_NLHE_DEPTH_MAX_ITERATIONS
        assert call(fn, 0, C.byref(a)) == _lib.RP_OK
        assert call(fn, 1, C.byref(a)) == _lib.RP_ERR_INVALID
        assert b"handle" in lib.rp_last_error()

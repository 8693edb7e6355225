"""CPU-side checks of the table-game subgame ABI (include/rp_mi355x.h: rp_mccfr_subgame_belief, rp_mccfr_subgame_solve and their _device
forms): the symbols exist, the five structs have the sizes the header states, the constants agree, and every argument a call is
refused for before a device is needed is refused, with the argument's name in rp_last_error."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from robopoker_amd import _lib, mccfr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rp_mi355x.h")
SYMBOLS = ("rp_mccfr_subgame_args_default", "rp_mccfr_subgame_belief", "rp_mccfr_subgame_belief_device", "rp_mccfr_subgame_solve",
           "rp_mccfr_subgame_solve_device")
SIZES = {"rp_mccfr_subgame_prior": 104, "rp_mccfr_subgame_entry": 140, "rp_mccfr_subgame_args": 32, "rp_mccfr_subgame_result": 192,
         "rp_mccfr_subgame_row": 264}
SOLVES = ("rp_mccfr_subgame_solve", "rp_mccfr_subgame_solve_device")
BELIEFS = ("rp_mccfr_subgame_belief", "rp_mccfr_subgame_belief_device")


def defaults():
    a = _lib.MccfrSubgameArgs()
    _lib.load().rp_mccfr_subgame_args_default(C.byref(a))
    return a


def test_symbols_exist():
    lib = _lib.load()
    text = open(HEADER).read()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.declared_symbols()
        assert re.search(r"RP_API (int|void) %s\(" % name, text)


def test_struct_sizes_are_the_headers(tmp_path):
    text = open(HEADER).read()
    for name, size in SIZES.items():
        m = re.search(r"\}\s*%s;\s*/\*\s*(\d+) bytes\s*\*/" % name, text)
        assert m and int(m.group(1)) == size, f"{name}: the header states {m and m.group(1)}"
    assert C.sizeof(_lib.MccfrSubgameArgs) == 32
    assert (mccfr.SUBGAME_PRIOR_DTYPE.itemsize, mccfr.SUBGAME_ENTRY_DTYPE.itemsize, mccfr.SUBGAME_RESULT_DTYPE.itemsize,
            mccfr.SUBGAME_ROW_DTYPE.itemsize) == (104, 140, 192, 264)
    offsets = {"rp_mccfr_subgame_entry": {f: mccfr.SUBGAME_ENTRY_DTYPE.fields[f][1] for f in ("candidate", "secret", "world_of", "harvest_order", "weights", "external")},
               "rp_mccfr_subgame_result": {f: mccfr.SUBGAME_RESULT_DTYPE.fields[f][1] for f in ("refined", "visits", "regret", "nodes", "drawn", "fallbacks")},
               "rp_mccfr_subgame_prior": {f: mccfr.SUBGAME_PRIOR_DTYPE.fields[f][1] for f in ("secret", "path", "n_prior", "n_worlds")},
               "rp_mccfr_subgame_row": {f: mccfr.SUBGAME_ROW_DTYPE.fields[f][1] for f in ("info", "enc")}}
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    if cc is not None:
        src = tmp_path / "sizes.c"
        lines = ['#include <stddef.h>\n#include "rp_mi355x.h"\n'] + [f'_Static_assert(sizeof({n}) == {b}, "{n}");\n' for n, b in SIZES.items()]
        lines += [f'_Static_assert(offsetof({n}, {f}) == {o}, "{n}.{f}");\n' for n, fs in offsets.items() for f, o in fs.items()]
        src.write_text("".join(lines))
        subprocess.check_call([cc, "-std=c11", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)])


def test_constants_are_the_headers():
    text = open(HEADER).read()
    assert "#define RP_MCCFR_SUBGAME_MAX_ITERATIONS (1u << 20)" in text and _lib.RP_MCCFR_SUBGAME_MAX_ITERATIONS == 1 << 20
    for name in ("RP_MCCFR_SUBGAME_MAX_NODES", "RP_MCCFR_SUBGAME_MAX_ROWS", "RP_MCCFR_SUBGAME_MAX_INFOS", "RP_MCCFR_SUBGAME_MAX_CANDIDATES"):
        m = re.search(r"#define %s (\d+)u" % name, text)
        assert m and int(m.group(1)) == getattr(_lib, name), name
    enum = re.search(r"enum \{ (RP_MSUB_OK = 0,[^}]*)\}", text).group(1)
    for item in enum.split(","):
        name, value = item.split("=")
        assert getattr(_lib, name.strip()) == int(value), name
    a = defaults()
    assert (a.iterations, a.prior, a.seed, a.first_id, a.rows_cap, a.reserved) == (1, 16384.0, 0, 0, 0, 0)
    _lib.load().rp_mccfr_subgame_args_default(None)  # a NULL out is ignored


def bad_args():
    out = []
    for field, value, word in (("iterations", 0, b"iterations"), ("iterations", (1 << 20) + 1, b"iterations"), ("prior", 0.0, b"prior"),
                               ("prior", -1.0, b"prior"), ("prior", float("nan"), b"prior"), ("prior", float("inf"), b"prior"),
                               ("reserved", 1, b"reserved")):
        a = defaults()
        setattr(a, field, value)
        out.append((a, word))
    return out


@pytest.mark.parametrize("form", SOLVES)
def test_solve_checks_args_first_without_a_device(form):
    fn = getattr(_lib.load(), form)
    buf = np.zeros(1024, np.uint8).ctypes.data
    assert fn(None, 1, None, None, None, None) == _lib.RP_ERR_INVALID and b"args is NULL" in _lib.load().rp_last_error()
    for a, word in bad_args():
        for n in (0, 1):  # args are checked whatever else is passed, n = 0 included
            assert fn(None, n, buf, C.byref(a), buf, None) == _lib.RP_ERR_INVALID
            assert word in _lib.load().rp_last_error()
    a = defaults()
    assert fn(None, 0, None, C.byref(a), None, None) == _lib.RP_OK  # n = 0: no launch, nothing else is looked at
    a.iterations = 1 << 20
    assert fn(None, 0, None, C.byref(a), None, None) == _lib.RP_OK
    a = defaults()
    assert fn(None, 1, buf, C.byref(a), buf, None) == _lib.RP_ERR_INVALID and b"h is NULL" in _lib.load().rp_last_error()


@pytest.mark.parametrize("form", BELIEFS)
def test_belief_refusals_without_a_device(form):
    fn = getattr(_lib.load(), form)
    buf = np.zeros(1024, np.uint8).ctypes.data
    assert fn(None, 0, None, None, None, None) == _lib.RP_OK
    assert fn(None, 1, buf, buf, buf, None) == _lib.RP_ERR_INVALID and b"h is NULL" in _lib.load().rp_last_error()


def test_python_wrappers_build_the_records():
    from robopoker_amd import Game, games

    g = Game("kuhn")
    prior, entry = games.subgame_entry(g, (0, 5), (0, 1), external=1, reach=True)
    assert prior.dtype == mccfr.SUBGAME_PRIOR_DTYPE and entry.dtype == mccfr.SUBGAME_ENTRY_DTYPE
    # Card::ALL minus seat 0's J0: J1 Q0 Q1 K0 K1, secrets their ranks; K|XB's slots are [Fold, Call] and Call < Fold
    assert list(entry["secret"][0][:5]) == [0, 1, 1, 2, 2] and entry["n_candidates"][0] == 5 and prior["n_path"][0] == 2
    assert g.info_name(g.table.states[int(entry["observed"][0])].info) == "J|XB" and list(entry["harvest_order"][0][:2]) == [1, 0]
    assert int(entry["candidate"][0][4]) == int(entry["observed"][0])
    with pytest.raises(ValueError):
        games.subgame_entry(Game("leduc"), (0, 3), (0, 0, ("board", 4)), external=0, reach=True)
    _, e = games.subgame_entry(Game("leduc"), (0, 3), (0, 0, ("board", 4)), external=0)
    assert list(e["secret"][0][:4]) == [0, 0, 1, 2] and e["n_candidates"][0] == 4  # Q1 and the board K0 excluded

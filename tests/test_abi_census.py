"""CPU-side checks of the blueprint census ABI (include/rp_mi355x.h, rp_nlhe_table_census and the rp_census_* summaries): the symbols
exist, the structs have the sizes the header states and the offsets of the ctypes and numpy mirrors, NULL arguments are refused before
a device is needed, and the four host-only summaries answer hand-made records as tests/nlhe_census_model.py does."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

import nlhe_census_model as CM
from robopoker_amd import _lib, nlhe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rp_mi355x.h")
STRUCTS = {"rp_census_cell": (_lib.CensusCell, 104), "rp_census_entry": (_lib.CensusEntry, 32), "rp_census": (_lib.Census, 20800),
           "rp_census_totals": (_lib.CensusTotals, 64), "rp_census_street": (_lib.CensusStreet, 40), "rp_census_peaks": (_lib.CensusPeaks, 32),
           "rp_census_grid": (_lib.CensusGrid, 32)}
CALLS = ("rp_nlhe_table_census", "rp_nlhe_table_census_device", "rp_census_stats", "rp_census_street_stats", "rp_census_saturation",
         "rp_census_grid_usage")
F = np.float32


def test_symbols_exist():
    lib, text = _lib.load(), open(HEADER).read()
    for name in CALLS:
        assert re.search(r"RP_API\s+int\s+" + name + r"\s*\(", text) and hasattr(lib, name) and name in _lib.declared_symbols()
    # the profiled steps' node census keeps its name and its signature
    assert "rp_nlhe_census" in _lib.declared_symbols() and len(_lib._SIGNATURES["rp_nlhe_census"][1]) == 3


def test_struct_sizes_and_offsets(tmp_path):
    text = open(HEADER).read()
    for name, (mirror, size) in STRUCTS.items():
        m = re.search(r"\}\s*%s;\s*/\*\s*(\d+) bytes\s*\*/" % name, text)
        assert m and int(m.group(1)) == size == C.sizeof(mirror), name
        assert re.search(r"RP_STATIC_ASSERT\(sizeof\(%s\) == %d," % (name, size), text), name
    for dtype, mirror in ((nlhe.CENSUS_CELL_DTYPE, _lib.CensusCell), (nlhe.CENSUS_ENTRY_DTYPE, _lib.CensusEntry), (nlhe.CENSUS_DTYPE, _lib.Census)):
        assert dtype.itemsize == C.sizeof(mirror)
        assert {f: dtype.fields[f][1] for f in dtype.names} == {f: getattr(mirror, f).offset for f, _ in mirror._fields_}
    assert (nlhe.CENSUS_TOP, nlhe.CENSUS_SEGMENT) == (64, 65536)
    assert int(re.search(r"#define RP_NLHE_CENSUS_TOP (\d+)u", text).group(1)) == 64
    assert int(re.search(r"#define RP_NLHE_CENSUS_SEGMENT (\d+)u", text).group(1)) == 65536
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    if cc is not None:
        src = tmp_path / "sizes.c"
        src.write_text('#include <stddef.h>\n#include "rp_mi355x.h"\n' +
                       "".join(f'_Static_assert(sizeof({n}) == {b}, "{n}");\n' for n, (_, b) in STRUCTS.items()) +
                       "".join(f'_Static_assert(offsetof(rp_census, {f}) == {getattr(_lib.Census, f).offset}, "{f}");\n' for f, _ in _lib.Census._fields_))
        subprocess.check_call([cc, "-std=c11", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)])


def test_edge_names_follow_the_display():
    assert [nlhe.edge_name(c) for c in (1, 2, 3, 4, 5, 6, 9, 10, 15, 19)] == ["?", "F", "O", "*", "!", "2bb", "5bb", "1:4", "1:1", "3:1"]
    assert nlhe.edge_name(0) == "#0" and nlhe.edge_name(31) == "#31" and len(nlhe.EDGE_NAMES) == 20


def test_null_arguments_are_invalid():
    lib = _lib.load()
    rec = np.zeros((), nlhe.CENSUS_DTYPE)
    p = rec.ctypes.data_as(C.c_void_p)
    for name in ("rp_nlhe_table_census", "rp_nlhe_table_census_device"):
        assert getattr(lib, name)(None, p) == _lib.RP_ERR_INVALID and b"rp_nlhe_table_census" in lib.rp_last_error()
        assert getattr(lib, name)(None, None) == _lib.RP_ERR_INVALID
    n = C.c_uint32()
    grid = (_lib.CensusGrid * 160)()
    assert lib.rp_census_stats(None, C.byref(_lib.CensusTotals())) == lib.rp_census_stats(p, None) == _lib.RP_ERR_INVALID
    assert lib.rp_census_street_stats(None, (_lib.CensusStreet * 5)()) == lib.rp_census_street_stats(p, None) == _lib.RP_ERR_INVALID
    assert lib.rp_census_saturation(None, C.byref(_lib.CensusPeaks())) == lib.rp_census_saturation(p, None) == _lib.RP_ERR_INVALID
    assert lib.rp_census_grid_usage(None, grid, C.byref(n)) == lib.rp_census_grid_usage(p, None, C.byref(n)) == _lib.RP_ERR_INVALID
    assert lib.rp_census_grid_usage(p, grid, None) == _lib.RP_ERR_INVALID and b"rp_census_grid_usage" in lib.rp_last_error()


def same(a, b):
    """two summaries: equal integers and strings, equal float32 BITS"""
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return set(a) <= set(b) | {"edge"} and all(same(v, b[k]) for k, v in a.items() if k != "edge")
    if isinstance(a, (float, np.floating)) or isinstance(b, (float, np.floating)):
        return F(a).tobytes() == F(b).tobytes()
    return a == b


def check(rec):
    assert same(nlhe.census_stats(rec), CM.stats(rec))
    assert same(nlhe.census_street_stats(rec), CM.street_stats(rec))
    assert same(nlhe.census_saturation(rec), CM.saturation(rec))
    got, want = nlhe.census_grid_usage(rec), CM.grid_usage(rec)
    assert same([{**g, "street": "PFTR?".index(g["street"])} for g in got], want)
    assert [g["edge"] for g in got] == [nlhe.edge_name(g["code"]) for g in got]
    return got


def cell(rec, s, e, **kw):
    c = rec["cell"][s][e]
    for k, v in kw.items():
        c[k] = v
    for k in ("max_regret", "min_regret", "max_weight", "max_payoff", "min_payoff", "max_visits", "min_visits"):
        if k not in kw:
            c[k] = 1
    rec["infosets"][s] += 1


def test_an_empty_record_is_all_zero():
    rec = np.zeros((), nlhe.CENSUS_DTYPE)
    assert check(rec) == []
    st = nlhe.census_stats(rec)
    assert st["infosets"] == st["edges"] == st["max_visits"] == 0 and all(F(v).tobytes() == bytes(4) for k, v in st.items() if k.startswith(("avg", "m")))
    assert [s["street"] for s in nlhe.census_street_stats(rec)] == list("PFTR?")
    sat = nlhe.census_saturation(rec)
    assert sat["precision_f32"] == np.finfo(F).max and sat["weight_pct"] == 0 and sat["regret_pct"] == 0
    assert nlhe.census_cold(rec) == [] and nlhe.census_hot(rec, 5) == []


def test_a_cell_without_a_rated_row_sorts_last():
    rec = np.zeros((), nlhe.CENSUS_DTYPE)
    cell(rec, 1, 4, rows=3, rated=0, total=0.0, weight=0.0, regret=-6.0, payoff=1.0, visits=10, min_regret=-3, max_regret=-1)
    cell(rec, 1, 12, rows=4, rated=4, dominant=1, ratio=0.4, total=8.0, weight=2.0, regret=1e-3, payoff=2.0, visits=2 ** 40)
    cell(rec, 1, 2, rows=2, rated=1, dominant=0, ratio=1e-9, total=4.0, weight=1.0, regret=0.1, payoff=3.0, visits=1)
    got = check(rec)
    assert [g["code"] for g in got] == [12, 2, 4] and got[2]["avg_freq"] == 0 and got[2]["weighted_freq"] == 0
    assert got[0]["avg_freq"] == F(0.4 / 4) and got[0]["weighted_freq"] == F(0.25) and got[0]["n_dominant"] == 1 and got[0]["n_decisions_with_edge"] == 4
    assert nlhe.census_saturation(rec)["max_regret"] == 3 and nlhe.census_stats(rec)["avg_visits"] == F((2 ** 40 + 11) / 9)


def test_grid_order_with_a_tie_and_street_four():
    rec = np.zeros((), nlhe.CENSUS_DTYPE)
    for s, e, ratio in ((4, 19, 1.5), (4, 3, 1.5), (4, 31, 2.5), (0, 7, 0.5), (2, 5, 0.0), (4, 1, 1.5)):
        cell(rec, s, e, rows=5, rated=5, dominant=2, ratio=ratio, total=3.0, weight=1.0, regret=0.1, payoff=0.1, visits=5)
    cell(rec, 4, 2, rows=1)  # not rated: behind every rated cell of its street, whatever its code
    got = check(rec)
    assert [(g["street"], g["code"]) for g in got] == [("P", 7), ("T", 5), ("?", 31), ("?", 1), ("?", 3), ("?", 19), ("?", 2)]
    assert [g["edge"] for g in got] == ["3bb", "!", "#31", "?", "O", "3:1", "F"]
    per = nlhe.census_street_stats(rec)
    assert [p["edges"] for p in per] == [5, 0, 5, 0, 21] and per[4]["street"] == "?" and per[4]["infosets"] == 5
    assert per[1]["avg_regret"] == 0 and per[4]["avg_regret"] == F((0.1 + 0.1 + 0.1 + 0.1) / 21)


def test_lists_read_the_record():
    rec = np.zeros((), nlhe.CENSUS_DTYPE)
    rec["n_cold"], rec["n_hot"] = 2, 1
    rec["cold"][0] = (5, 6, 7, 2, 0, 0.0)
    rec["cold"][1] = (8, 9, 10, 3, 4, 0.0)
    rec["hot"][0] = (1, 2, 3, 4, 0, -2.5)
    assert nlhe.census_cold(rec) == [dict(past=5, present=7, choices=6, visits=0, edges=2), dict(past=8, present=10, choices=9, visits=4, edges=3)]
    assert nlhe.census_cold(rec, 1) == nlhe.census_cold(rec)[:1]
    assert nlhe.census_hot(rec) == [dict(past=1, present=3, choices=2, max_regret=F(-2.5), edges=4)]

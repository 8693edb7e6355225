"""CPU-side checks of the search-match ABI (include/rp_mi355x.h, rp_nlhe_search_match): the symbols exist, the two structs have the
sizes the header states, and the arguments a call is refused for are refused before a device is needed, in the header's order."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from robopoker_amd import _lib, nlhe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rp_mi355x.h")
STRUCTS = {"rp_nlhe_search_args": _lib.NlheSearchArgs, "rp_nlhe_search_step": _lib.NlheSearchStep}
FORMS = ("rp_nlhe_search_match", "rp_nlhe_search_match_device")


def call(fn, n, args, h0=None, h1=None, steps=None):
    return fn(h0, h1, n, args, None, None, None, None, None, None, steps)


def defaults():
    a = _lib.NlheSearchArgs()
    _lib.load().rp_nlhe_search_args_default(C.byref(a))
    return a


def test_symbols_exist():
    lib = _lib.load()
    for name in ("rp_nlhe_search_args_default",) + FORMS:
        assert hasattr(lib, name) and name in _lib.declared_symbols()


def test_struct_sizes_are_the_headers(tmp_path):
    text = open(HEADER).read()
    stated = {}
    for name, mirror in STRUCTS.items():
        m = re.search(r"\}\s*%s;\s*/\*\s*(\d+) bytes\s*\*/" % name, text)
        assert m, f"{name}: the header states no size"
        stated[name] = int(m.group(1))
        assert C.sizeof(mirror) == stated[name], name
    assert stated == {"rp_nlhe_search_args": 72, "rp_nlhe_search_step": 352}
    dtype, mirror = nlhe.SEARCH_STEP_DTYPE, _lib.NlheSearchStep
    assert dtype.itemsize == 352 and {f: dtype.fields[f][1] for f in dtype.names} == {f: getattr(mirror, f).offset for f, _ in mirror._fields_}
    assert _lib.NlheSearchArgs.match.offset == 0 and C.sizeof(_lib.NlheMatchArgs) == 32  # the match args lead, as they are
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    if cc is not None:
        src = tmp_path / "sizes.c"
        src.write_text('#include "rp_mi355x.h"\n' + "".join(f'_Static_assert(sizeof({n}) == {b}, "{n}");\n' for n, b in stated.items()))
        subprocess.check_call([cc, "-std=c11", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)])


def test_constants_are_the_headers():
    text = open(HEADER).read()
    assert int(re.search(r"#define RP_NLHE_SEARCH_MAX_SOLVES (\d+)u", text).group(1)) == _lib.RP_NLHE_SEARCH_MAX_SOLVES == 48
    assert re.search(r"RP_SEARCH_NONE = 0, RP_SEARCH_WORLD = 1", text) and _lib.SEARCH == {"none": 0, "world": 1}


def test_defaults_are_the_references():
    a, m, s = defaults(), _lib.NlheMatchArgs(), _lib.NlheSubgameArgs()
    _lib.load().rp_nlhe_match_args_default(C.byref(m))
    _lib.load().rp_nlhe_subgame_args_default(C.byref(s))
    assert bytes(a.match) == bytes(m)
    assert (a.iterations, a.rollouts, a.bias, a.prior) == (s.iterations, s.rollouts, s.bias, s.prior) == (1, 16, 5.0, 16384.0)
    assert (tuple(a.search), a.origin_mode, tuple(a.reserved0), a.visit_threshold, a.steps_cap, a.search_seed) == ((0, 0), 0, (0,) * 5, 1 << 18, 0, 0)


def bad(**kw):
    a = defaults()
    for k, v in kw.items():
        if k in ("agent", "stacks", "reserved"):
            for i, x in enumerate(v):
                getattr(a.match, k)[i] = x
        elif k in ("dealer", "hero", "mirror", "snap", "board_mode"):
            setattr(a.match, k, v)
        elif k in ("search", "reserved0"):
            for i, x in enumerate(v):
                getattr(a, k)[i] = x
        else:
            setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,word", [
    (dict(agent=(3, 0)), b"agent"), (dict(dealer=3), b"dealer"), (dict(hero=2), b"hero"), (dict(mirror=2), b"mirror"), (dict(snap=2), b"snap"),
    (dict(board_mode=2), b"board_mode"), (dict(stacks=(0, 5)), b"stacks"), (dict(stacks=(-1, 5)), b"stacks"), (dict(reserved=(0, 0, 1)), b"reserved"),
    (dict(search=(2, 0)), b"search"), (dict(search=(0, 2)), b"search"), (dict(search=(1, 0), agent=(2, 0)), b"fish"),
    (dict(search=(0, 1), agent=(0, 2)), b"fish"), (dict(origin_mode=2), b"origin_mode"), (dict(visit_threshold=0), b"visit_threshold"),
    (dict(iterations=0), b"iterations"), (dict(iterations=_lib.RP_NLHE_DEPTH_MAX_ITERATIONS + 1), b"iterations"), (dict(rollouts=4097), b"rollouts"),
    (dict(bias=0.0), b"bias"), (dict(bias=float("nan")), b"bias"), (dict(prior=float("inf")), b"prior"), (dict(prior=-1.0), b"prior"),
    (dict(reserved0=(0, 0, 0, 0, 1)), b"reserved"), (dict(steps_cap=1), b"steps")])
def test_bad_args_are_invalid(kw, word):
    lib = _lib.load()
    a = bad(**kw)
    for name in FORMS:
        for n in (0, 1):
            assert call(getattr(lib, name), n, C.byref(a)) == _lib.RP_ERR_INVALID
            assert word in lib.rp_last_error() and b"rp_nlhe_search_match" in lib.rp_last_error()


def test_the_order_of_the_refusals():
    lib = _lib.load()
    for name in FORMS:
        fn = getattr(lib, name)
        assert call(fn, 1, C.byref(bad(dealer=3, search=(2, 0), visit_threshold=0))) == _lib.RP_ERR_INVALID and b"dealer" in lib.rp_last_error()
        assert call(fn, 1, C.byref(bad(search=(2, 0), visit_threshold=0, iterations=0))) == _lib.RP_ERR_INVALID and b"search" in lib.rp_last_error()
        # seat 1's kind is refused before seat 0's fish: both kinds are looked at first
        assert call(fn, 1, C.byref(bad(search=(1, 2), agent=(2, 0)))) == _lib.RP_ERR_INVALID and b"rp_search_kind" in lib.rp_last_error()
        assert call(fn, 1, C.byref(bad(search=(1, 0), agent=(2, 0), origin_mode=2))) == _lib.RP_ERR_INVALID and b"fish" in lib.rp_last_error()
        assert call(fn, 1, C.byref(bad(origin_mode=2, visit_threshold=0))) == _lib.RP_ERR_INVALID and b"origin_mode" in lib.rp_last_error()
        assert call(fn, 1, C.byref(bad(visit_threshold=0, iterations=0))) == _lib.RP_ERR_INVALID and b"visit_threshold" in lib.rp_last_error()
        assert call(fn, 1, C.byref(bad(iterations=0, reserved0=(1,)))) == _lib.RP_ERR_INVALID and b"iterations" in lib.rp_last_error()


def test_null_args_and_an_empty_batch():
    lib = _lib.load()
    for name in FORMS:
        fn, a = getattr(lib, name), defaults()
        assert call(fn, 0, None) == _lib.RP_ERR_INVALID
        assert call(fn, 0, C.byref(a)) == _lib.RP_OK  # n = 0: no launch, nothing is looked at, not even the handles
        a.search[0], a.rollouts, a.iterations = 1, 0, _lib.RP_NLHE_DEPTH_MAX_ITERATIONS  # rollouts 0 reads as 1
        assert call(fn, 0, C.byref(a)) == _lib.RP_OK
        assert call(fn, 1, C.byref(a)) == _lib.RP_ERR_INVALID
        assert b"handle" in lib.rp_last_error()

"""CPU-side checks of the table-game depth-limited ABI (include/rp_mi355x.h: rp_mccfr_set_frontiers, rp_game_frontiers,
rp_mccfr_depth_solve and its _device form): the symbols and constants, rp_game_frontiers for the four built-in games against
hand-written rules, and every refusal that needs no device, with the field's name in rp_last_error."""
import ctypes as C
import re
import os

import numpy as np
import pytest

import mccfr_subgame_model as M
from robopoker_amd import Game, _lib, games, mccfr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rp_mi355x.h")
SYMBOLS = ("rp_mccfr_set_frontiers", "rp_game_frontiers", "rp_mccfr_depth_solve", "rp_mccfr_depth_solve_device")
SOLVES = ("rp_mccfr_depth_solve", "rp_mccfr_depth_solve_device")


def test_symbols_constants_and_layout():
    lib, text = _lib.load(), open(HEADER).read()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.declared_symbols()
        assert re.search(r"RP_API int %s\(" % name, text)
    assert "#define RP_MCCFR_ORIGIN_ENTRY 254u" in text and _lib.RP_MCCFR_ORIGIN_ENTRY == 254
    assert "#define RP_MCCFR_ORIGIN_NONE  255u" in text and _lib.RP_MCCFR_ORIGIN_NONE == 255
    assert "RP_MSUB_FRONTIER = 13" in text and _lib.RP_MSUB_FRONTIER == 13
    assert C.sizeof(_lib.MccfrFrontiers) == 4 * C.sizeof(C.c_void_p) + 16
    # the two bytes the depth-limited call gave a meaning keep their places: kind after n_actions, frontiers after fallbacks
    assert mccfr.SUBGAME_ROW_DTYPE.fields["kind"][1] == 2 and mccfr.SUBGAME_ROW_DTYPE.fields["info"][1] == 4
    assert mccfr.SUBGAME_RESULT_DTYPE.fields["frontiers"][1] == 188 and mccfr.SUBGAME_RESULT_DTYPE.itemsize == 192


@pytest.mark.parametrize("kind", ["kuhn", "rps"])
def test_games_without_depth_have_no_frontier(kind):
    g = Game(kind)
    f = games.frontiers(g)
    assert f["n_pick"] == 0 and not f["depth"].any()
    assert (f["pick_info"] == _lib.RP_NO_INFO).all() and (f["payoff_ref"] == _lib.RP_NO_INFO).all()
    assert f["depth"].shape == (g.table.n_states,)


@pytest.mark.parametrize("kind,cards", [("leduc", 6), ("leduc_wide", 14)])
def test_leduc_depth_and_pick_ids(kind, cards):
    """depth by a hand-written rule: 0 at Start, Dealt and the round-1 decisions, 1 at the board deal, in round 2 and at every
    terminal (leduc/src/game.rs:232-237); one Pick id per (seat 0's rank, round-1 spot), shared exactly by the board-deal states equal
    in both, numbered by the lowest-numbered state that carries them"""
    g = Game(kind)
    t, f = M.Table(g.table), games.frontiers(g)
    want_depth, keys = np.zeros(t.n_states, np.uint8), {}

    def walk(s, depth, c0, spot):
        """spot: the round-1 actions so far, while round 1 lasts"""
        if t.turn[s] == M.TERMINAL or (t.turn[s] == M.CHANCE and spot is not None):
            depth = 1  # Over(_), Deal(_): and everything below
        want_depth[s] = depth
        if t.turn[s] == M.CHANCE and spot is not None and depth == 1 and s not in keys and len(t.kids[s]) == cards - 2:
            keys[s] = (c0 // 2, spot)
        for k, c in enumerate(t.kids[s]):
            walk(c, depth, c0, None if depth == 1 else spot + (k,))

    for c0 in range(cards):
        dealt = t.kids[0][c0]
        for first in t.kids[dealt]:
            walk(first, 0, c0, ())
    assert np.array_equal(f["depth"], want_depth)
    assert want_depth[0] == 0 and all(want_depth[s] == 0 for s in t.kids[0])
    boards = [s for s in range(t.n_states) if s in keys]
    assert len(boards) == cards * (cards - 1) * 3 and f["n_pick"] == (cards // 2) * 3
    ids = {}
    for s in boards:  # ascending state number: a new key takes the next id
        ids.setdefault(keys[s], len(ids))
        assert f["pick_info"][s] == ids[keys[s]], (s, keys[s])
    others = np.ones(t.n_states, bool)
    others[boards] = False
    assert (f["pick_info"][others] == _lib.RP_NO_INFO).all() and (f["payoff_ref"] == _lib.RP_NO_INFO).all()
    assert all(t.turn[s] == M.CHANCE and f["depth"][s] == 1 for s in boards)


def test_game_frontiers_refuses_null():
    lib, g = _lib.load(), Game("kuhn")
    buf = np.zeros(4 * g.table.n_states, np.uint8).ctypes.data
    n = C.c_uint32()
    assert lib.rp_game_frontiers(None, buf, buf, buf, C.byref(n)) == _lib.RP_ERR_INVALID
    assert lib.rp_game_frontiers(g._h, buf, None, buf, C.byref(n)) == _lib.RP_ERR_INVALID
    assert lib.rp_game_frontiers(g._h, buf, buf, buf, None) == _lib.RP_ERR_INVALID and b"rp_game_frontiers" in lib.rp_last_error()


def tables(n=8, matrices=None, **fields):
    leaves = 2
    depth, pick, ref = np.zeros(n, np.uint8), np.full(n, _lib.RP_NO_INFO, np.uint32), np.full(n, _lib.RP_NO_INFO, np.uint32)
    mats = np.zeros((1, leaves, leaves), np.float32) if matrices is None else np.asarray(matrices, np.float32)
    f = _lib.MccfrFrontiers(depth.ctypes.data, pick.ctypes.data, ref.ctypes.data, mats.ctypes.data, 1, len(mats), leaves, 0)
    for k, v in fields.items():
        setattr(f, k, v)
    return f, (depth, pick, ref, mats)


def test_set_frontiers_checks_its_own_fields_before_the_handle():
    """leaves, reserved, a NULL array, n_pick and the matrix entries need neither a handle nor a device: they are refused with a NULL
    handle, by name; well-formed tables with a NULL handle name the handle"""
    lib = _lib.load()
    bad = np.zeros((2, 2, 2), np.float32)
    for word, (f, keep) in ((b"leaves", tables(leaves=0)), (b"leaves", tables(leaves=5)),
                            (b"reserved", tables(reserved=1)), (b"depth is NULL", tables(depth=None)), (b"pick_info is NULL", tables(pick_info=None)),
                            (b"payoff_ref is NULL", tables(payoff_ref=None)), (b"matrices is NULL", tables(n_matrices=1)),
                            (b"n_pick", tables(n_pick=_lib.RP_MCCFR_SUBGAME_MAX_INFOS + 1))):
        if word == b"matrices is NULL":
            f.matrices = None
        assert lib.rp_mccfr_set_frontiers(None, C.byref(f)) == _lib.RP_ERR_INVALID and word in lib.rp_last_error(), (word, lib.rp_last_error())
    for value, cell in ((np.nan, (1, 0, 1)), (np.inf, (0, 1, 1)), (-np.inf, (1, 1, 0))):
        m = bad.copy()
        m[cell] = value
        f, keep = tables(matrices=m)
        assert lib.rp_mccfr_set_frontiers(None, C.byref(f)) == _lib.RP_ERR_INVALID
        assert b"matrices[%d][%d][%d] is not finite" % cell in lib.rp_last_error(), lib.rp_last_error()
    f, keep = tables(n_pick=_lib.RP_MCCFR_SUBGAME_MAX_INFOS, matrices=np.full((3, 2, 2), 3.4e38, np.float32))
    assert lib.rp_mccfr_set_frontiers(None, C.byref(f)) == _lib.RP_ERR_INVALID and b"h is NULL" in lib.rp_last_error()
    assert lib.rp_mccfr_set_frontiers(None, None) == _lib.RP_ERR_INVALID and b"h is NULL" in lib.rp_last_error()


def defaults():
    a = _lib.MccfrSubgameArgs()
    _lib.load().rp_mccfr_subgame_args_default(C.byref(a))
    return a


@pytest.mark.parametrize("form", SOLVES)
def test_depth_solve_checks_args_first_without_a_device(form):
    """rp_mccfr_subgame_solve's checks in their order: args, n = 0, the handle"""
    fn, lib = getattr(_lib.load(), form), _lib.load()
    buf = np.zeros(1024, np.uint8).ctypes.data
    assert fn(None, 1, None, None, None, None, None) == _lib.RP_ERR_INVALID and b"args is NULL" in lib.rp_last_error()
    for field, value, word in (("iterations", 0, b"iterations"), ("iterations", (1 << 20) + 1, b"iterations"), ("prior", 0.0, b"prior"),
                               ("prior", float("nan"), b"prior"), ("reserved", 1, b"reserved")):
        a = defaults()
        setattr(a, field, value)
        for n in (0, 1):
            assert fn(None, n, buf, buf, C.byref(a), buf, None) == _lib.RP_ERR_INVALID and word in lib.rp_last_error()
    a = defaults()
    assert fn(None, 0, None, None, C.byref(a), None, None) == _lib.RP_OK
    assert fn(None, 1, buf, None, C.byref(a), buf, None) == _lib.RP_ERR_INVALID and b"rp_mccfr_depth_solve: h is NULL" in lib.rp_last_error()


def test_python_wrappers_build_the_records():
    g = Game("leduc")
    e = games.depth_entry(g, (0, 3), (0,), internal=1)
    assert e.dtype == mccfr.SUBGAME_ENTRY_DTYPE and e.shape == (1,)
    assert (int(e["observed"][0]), int(e["external"][0]), int(e["n_candidates"][0]), int(e["n_worlds"][0])) == (games.play(g, (0, 3), (0,)), 0, 0, 1)
    assert list(e["weights"][0]) == [1, 0, 0, 0] and (e["world_of"][0] == _lib.RP_WORLD_NONE).all() and e["harvest_info"][0] == _lib.RP_NO_INFO
    assert mccfr.Solver._origin(None, 3) is None and list(mccfr.Solver._origin(0, 2)) == [0, 0]
    assert list(mccfr.Solver._origin([1, None, _lib.RP_MCCFR_ORIGIN_NONE], 3)) == [1, 254, 255]
    with pytest.raises(ValueError):
        mccfr.Solver._origin([0, 1], 3)
    with pytest.raises(ValueError):
        games.depth_entry(Game("rps"), (0, 1))

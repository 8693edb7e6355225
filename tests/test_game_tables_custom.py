"""Caller-built game tables (tests/game_tables.py) on the host: what rp_game_table_check accepts and refuses, and the oracle on
those tables against an independent enumeration and against exactly restated chance draws.  No device involved; the device side
of the same tables is tests/test_gpu_mccfr_tables.py."""
import ctypes as C

import numpy as np
import pytest

import game_tables as GT
import oracle
from mccfr_hand import chance_draw, hand_decisions, sampled_trees
from robopoker_amd import _lib


def _check(table):
    return _lib.load().rp_game_table_check(C.byref(table))


def _last_error():
    return _lib.load().rp_last_error().decode()


# ---- accepted tables ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GT.CATALOGUE))
def test_catalogue_tables_pass_the_check_and_their_bounds_are_the_librarys(name):
    # the bounds are computed in Python (TableGame.bounds); the library derives its own in csrc/games.cpp.  They are compared at the
    # acceptance edge: declaring exactly the Python value is accepted, one less is refused — so the two are equal
    g = GT.game(name)
    assert _check(g.table) == _lib.RP_OK, _last_error()
    assert _check(g.make_table(max_depth=g.max_depth - 1)) == _lib.RP_ERR_INVALID
    assert "max_depth" in _last_error()
    assert _check(g.make_table(max_tree_nodes=g.max_tree_nodes - 1)) == _lib.RP_ERR_INVALID
    assert "max_tree_nodes" in _last_error()
    # overstating stays legal
    assert _check(g.make_table(max_depth=g.max_depth + 3, max_tree_nodes=g.max_tree_nodes + 40)) == _lib.RP_OK


def test_the_catalogue_sits_on_the_limits_of_the_lds_traversal():
    # the pairs differ in ONE quantity, which is at the LDS traversal's limit in the first game and one past it in the second
    # (mccfr.hip traverse_fits_lds: 62 nodes, 32 internal nodes, depth 10, 8191 infosets); everything else is well inside
    b = {name: GT.game(name).bounds() for name in GT.CATALOGUE}
    assert (b["depth10"]["depth"], b["depth11"]["depth"]) == (10, 11)
    assert (b["nodes62"]["nodes"], b["nodes63"]["nodes"]) == (62, 63)
    assert (b["internal32"]["internal"], b["internal33"]["internal"]) == (32, 33)
    assert (GT.game("infos8191").n_infos, GT.game("infos8192").n_infos) == (8191, 8192)
    for name, over in (("depth11", "depth"), ("nodes63", "nodes"), ("internal33", "internal")):
        limits = dict(depth=10, nodes=62, internal=32)
        assert all(b[name][k] <= v for k, v in limits.items() if k != over), (name, b[name])
        assert GT.game(name).n_infos <= 8191
    assert b["infos8192"]["depth"] <= 10 and b["infos8192"]["nodes"] <= 62 and b["infos8192"]["internal"] <= 32
    for name, entry in GT.CATALOGUE.items():
        assert GT.game(name).expected_variant() == entry["variant"], name
    # the shapes the table of the catalogue promises
    g = GT.game("three_players_a5")
    assert g.n_players == 3 and sorted(set(g.info_actions)) == [1, 2, 3, 5] and set(g.info_player) == {0, 1, 2}
    w = GT.game("widest_a16")
    assert w.max_actions == 16 and w.n_infos >= 300 and w.table.default_regret and np.count_nonzero(w.default_regret) > w.n_infos
    assert GT.game("one_player").n_players == 1 and len(GT.game("two_states").turn) == 2
    mid = GT.game("chance16_mid")
    wide = [s for s in range(len(mid.turn)) if mid.turn[s] == GT.CHANCE and mid.nch[s] == 16]
    assert wide and all(mid.chance_info[s] for s in wide)
    parent = {c: s for s in range(len(mid.turn)) for c in mid.children[mid.offset[s]:mid.offset[s] + mid.nch[s]]}
    assert all(mid.turn[parent[s]] == 0 and mid.turn[mid.children[mid.offset[s]]] == 1 for s in wide)
    # payoffs are not zero-sum
    t = g.table
    assert any(sum(t.payoffs[r * 3 + p] for p in range(3)) != 0 for r in range(t.n_terminals))


# ---- rejected tables -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[17, 255])
def wide_chance(request):
    return GT.TableGame(2, [("chance", request.param), ("act", 0, 2)], seed=request.param)


def test_a_chance_node_wider_than_16_is_refused_with_the_state_and_the_limit(wide_chance):
    assert _check(wide_chance.table) == _lib.RP_ERR_CAPACITY
    msg = _last_error()
    assert "state 0" in msg and "16" in msg and str(wide_chance.nch[0]) in msg
    # 16 outcomes are held
    assert _check(GT.game("chance16_root").table) == _lib.RP_OK


def test_the_oracle_refuses_the_same_wide_tables(wide_chance):
    hp = oracle.default_hyper()
    h = oracle.load().ora_mccfr_create(C.byref(wide_chance.table), 0, 0, 0, 8, C.byref(hp), 1)
    assert not h


def test_a_wide_chance_node_below_the_root_is_refused_too():
    g = GT.TableGame(2, [("act", 0, 2), ("chance", lambda pub: 17 if pub[-1][1] == 1 else 3), ("act", 1, 2)])
    assert _check(g.table) == _lib.RP_ERR_CAPACITY
    state = next(s for s in range(len(g.turn)) if g.nch[s] == 17)
    assert f"state {state} " in _last_error()


@pytest.mark.parametrize("name", ["three_players_a5", "depth11", "nodes63"])
def test_understated_bounds_are_refused_before_anything_is_launched(name):
    g = GT.game(name)
    for field in ("max_depth", "max_tree_nodes"):
        for declared in (0, 1, getattr(g, field) - 1):
            assert _check(g.make_table(**{field: declared})) == _lib.RP_ERR_INVALID, (field, declared)


def test_the_built_in_games_declare_their_true_bounds():
    # rp_game_create fills the fields with the recursion the check runs: exact, so one less is refused
    from robopoker_amd import Game

    for kind in ("kuhn", "leduc", "rps", "leduc_wide"):
        g = Game(kind)
        assert _check(g.table) == _lib.RP_OK
        for field in ("max_depth", "max_tree_nodes"):
            t = _lib.GameTable()
            C.memmove(C.byref(t), C.byref(g.table), C.sizeof(t))
            setattr(t, field, getattr(t, field) - 1)
            assert _check(t) == _lib.RP_ERR_INVALID, (kind, field)


# ---- the oracle against the independent enumeration --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three_players_a5", "one_player", "two_states"])
def test_first_batch_decisions_of_every_walker_are_hand_traceable(name):
    # tests/mccfr_hand.py enumerates every tree external sampling can produce for a walker and the regret vector / expected value of
    # each walker infoset in it under a fresh profile (exact rationals).  Every Decisions of the oracle's batch at epoch w (walker
    # w % n_players) must be one of them, whatever its RNG drew.  A fresh profile at epoch w: zero rows loaded at that epoch.
    g = GT.game(name)
    fresh = np.zeros(g.n_infos * g.max_actions, dtype=oracle.ENC_DTYPE)
    for walker in range(g.n_players):
        allowed = set()
        for tree in sampled_trees(g, walker):
            for info, regrets, ev in hand_decisions(g, tree, walker):
                allowed.add((info, tuple(round(r, 5) for r in regrets), round(ev, 5)))
        s = oracle.OracleSolver(g, "summed", "constant", "external", batch=400, seed=5 + walker)
        s.load_rows(fresh, epoch=walker)
        assert s.epoch == walker
        decs = s.batch()
        owners = {g.player(d["info"]) for d in decs}
        if any(p == walker for p in g.info_player):
            assert owners == {walker}
        else:
            assert decs == []  # a player without a decision: the batch is empty
        for d in decs:
            assert d["n"] == g.n_actions(d["info"]) and d["expanded"] == (1 << d["n"]) - 1
            key = (d["info"], tuple(round(r, 5) for r in d["regret"]), round(d["payoff"], 5))
            assert key in allowed, (walker, key)
        # ... and the step applies exactly that batch (Summed: R += delta; every edge of a decided infoset is visited once)
        s.step()
        rows = s.export().reshape(g.n_infos, g.max_actions)
        want = np.zeros((g.n_infos, g.max_actions))
        seen = np.zeros((g.n_infos, g.max_actions), dtype=np.uint32)
        for d in decs:
            want[d["info"], :d["n"]] += d["regret"]
            seen[d["info"], :d["n"]] += 1
        assert np.allclose(rows["regret"], want, rtol=1e-5, atol=1e-5)
        assert np.array_equal(rows["visits"], seen)


# ---- chance draws: exact counts ----------------------------------------------------------------------------------------------------
def chance_draw_reference(g, seed, batch):
    """per outcome k of the 16-way root chance of "chance16_root": how many tree ids of the first batch draw k under the restated
    rp_node_hash / rp_pick_uniform (tests/mccfr_hand.py), and the infoset below outcome k"""
    want = [0] * 16
    for tree in range(batch):
        want[chance_draw(seed, 0, tree, 0, 16)] += 1
    return want, [g.info_of((0, 1, ((0, k),), ())) for k in range(16)]


def test_the_oracles_16_way_chance_draws_are_the_restated_ones_exactly():
    # no statistical margin: after one step the infoset below outcome k has been visited once per tree that drew k
    g = GT.game("chance16_root")
    seed, batch = 3, 4000
    want, infos = chance_draw_reference(g, seed, batch)
    assert min(want) > 0 and sum(want) == batch  # every outcome is drawn, the 16th included
    s = oracle.OracleSolver(g, "linear", "linear", "external", batch=batch, seed=seed)
    s.step()
    rows = s.export().reshape(g.n_infos, g.max_actions)
    assert [int(rows["visits"][i, 0]) for i in infos] == want
    assert [int(rows["visits"][i, 1]) for i in infos] == want

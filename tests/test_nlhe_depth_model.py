"""Pins the model of the depth-limited re-solve (tests/nlhe_depth_model.py) without a GPU: one iteration of a three-leaf river tree
against regrets worked out by hand, the shape the frontier game takes in a tree, chance leaves valued by stored payoffs under
origin = street, and the properties the header promises (determinism in (seed, first_id + i), a T-iteration solve being the first T
iterations of a longer one).

The frontier game, as the reference's sources have it (subgame/src/depth/encoder.rs:93-121, game.rs:73-77, mccfr/src/sample/external.rs):
DepthEncoder::branches turns a COPY of the node's game into the Frontier phase, so the node the tree stores is still the chance node it
was grown as.  ExternalSampling therefore keeps one of its four Pick branches (`randomly`), its own info is DepthInfo::Game and is never
read, and the Pick infoset holds the one Internal(k) node alone: a one-node span whose head's turn is the seat opposite `internal`.  It
is updated when that seat is the walker and dropped when `internal` is.  A five-node Pick span (the frontier node and four Internal
children under one infoset) would need the stored node to be in the Frontier phase, which no code path produces; the tests below pin
what the sources do."""
import ctypes as C

import numpy as np
import pytest

import nlhe_depth_model as DM
import nlhe_policy_model as PM
import nlhe_rollout_model as FM
import oracle_nlhe as ON
from robopoker_amd.nlhe import Frontier

F = np.float32
EPS = PM.EPSILON
OPEN2, POT, HALF = ON.Open(2), ON.RaiseOdds(1, 1), ON.RaiseOdds(1, 2)
DRAW, FOLD, CHECK, CALL, SHOVE = ON.E_DRAW, ON.E_FOLD, ON.E_CHECK, ON.E_CALL, ON.E_SHOVE


def cards(*cs):
    return sum(1 << c for c in cs)


HOLES, FLOP, TURN, RIVER = (cards(51, 50), cards(12, 25)), cards(3, 17, 30), cards(44), cards(9)
FLOP_ENTRY = Frontier(HOLES, 0, [FLOP], [OPEN2, CALL, DRAW])
KW = dict(rollouts=2, bp_epoch=3, prior=64.0, seed=11, first_id=5)


class Empty:
    """a blueprint without a row"""

    def enc(self, key):
        return None

    get = enc


class Fixed(DM.Blueprint):
    """DM.Blueprint with every infoset present"""

    def enc(self, key):
        row = super().enc(key)
        if row is None:
            row = self.loaded[key] = np.zeros(DM.A, DM.ENC)
            row["weight"], row["regret"], row["visits"] = 1.0, 2.5, 4
            row["payoff"] = np.arange(DM.A, dtype=F) + F(0.75)
        return row


def payoff(g, seat):
    out = C.c_float()
    assert ON.lib().ora_nlhe_payoff(C.byref(g), seat, C.byref(out)) == 0
    return F(out.value)


def after(g, edge):
    o, g = ON.lib(), FM._copy(g)
    assert o.ora_nlhe_apply(C.byref(g), C.byref(o.ora_nlhe_snap(C.byref(g), o.ora_nlhe_actionize(C.byref(g), edge, 0)))) == 0
    return g


def test_one_iteration_of_a_river_tree_by_hand():
    """Seat 0 faces a pot bet on the river with 15 chips behind, seat 1 has 5: the choices are Shove, Call, Fold, and a shove leaves seat 1
    with Shove or Fold.  No chance node; an empty blueprint, so every infoset reads as the defaults (Shove 0, Call 50, Fold 100)."""
    entry = Frontier(HOLES, 0, [FLOP, TURN, RIVER], [OPEN2, CALL, DRAW, CHECK, CHECK, DRAW, CHECK, CHECK, DRAW, POT], [POT], stacks=(20, 20))
    keep = []
    got = DM.solve(entry, None, Empty(), 0, 1, keep=keep, **KW)
    s = keep[0]
    tree = s.trees[0]
    assert got["status"] == DM.OK and got["frontiers"] == 0 and got["nodes"] == 5 and got["infosets"] == 1 and got["n_rows"] == 1
    # the builder's order: the root's branches are pushed Shove, Call, Fold and grown from the top of the stack
    assert [(n.edge, n.parent.index if n.parent else None) for n in tree[:4]] == [(None, None), (FOLD, 0), (CALL, 0), (SHOVE, 0)]
    assert list(PM.edges(tree[0].info[3])[:3]) == [SHOVE, CALL, FOLD] and list(PM.edges(tree[3].info[3])[:2]) == [SHOVE, FOLD]
    g = FM.frontier_game(entry)
    v_fold, v_call = payoff(after(g, FOLD), 0), payoff(after(g, CALL), 0)
    assert v_fold == F(-5.0)
    # seat 1's node is sampled: weights EPSILON each -> ((EPS / 1 + 2) / (2 EPS + 2)) = 1 each, z = 2, q = 1/2 each; the draw of node 3
    u = FM.u01(FM.node_hash(KW["seed"], DM.DRAW_EPOCH, KW["first_id"] * DM.MAX_ITERATIONS, 3))
    pick = SHOVE if F(0.5) > u else FOLD
    assert tree[4].edge == pick and tree[4].parent is tree[3]
    sigma = F(EPS / F(100.0)) if pick == SHOVE else F(F(100.0) / F(100.0))  # regret() / (EPS + 100)
    v_shove = F(F(1.0) * F(F(sigma / F(0.5)) * payoff(after(after(g, SHOVE), pick), 0)))
    rd = F(F(EPS + F(50.0)) + F(100.0))
    assert rd == F(150.0)
    ev = F(F(F(F(0.0) + F(F(EPS / rd) * v_shove)) + F(F(F(50.0) / rd) * v_call)) + F(F(F(100.0) / rd) * v_fold))
    want_regret = [F(EPS + F(v_shove - ev)), F(F(50.0) + F(v_call - ev)), F(F(100.0) + F(v_fold - ev))]
    third = F(EPS / F(F(EPS + EPS) + EPS))
    want_weight = F(F(F(third * F(64.0)) * F(65.0)) / F(2.0))  # warmstart; + policy * 0 at t = 0
    kind, n_actions, past, present, choices, enc = got["rows"][0]
    assert (kind, n_actions, past, choices) == (DM.GAME, 3, ON.path_pack([POT]), tree[0].info[3])
    assert [x.tobytes() for x in enc["regret"][:3]] == [x.tobytes() for x in want_regret]
    assert (enc["weight"][:3] == want_weight).all() and (enc["payoff"][:3] == ev).all() and (enc["visits"][:3] == 1).all()
    assert not enc[3:].view(np.uint8).any()
    # the harvest reads the local row
    assert np.array_equal(got["refined"][:3], PM.distribution("iterated", list(want_regret) + [0] * 6, 3)[:3])
    assert got["regret"] == DM.fold(np.fmax(x, F(0.0)) for x in want_regret) == got["sum_regret"]


def test_the_frontier_game_in_a_tree():
    """one Internal(k) node below every frontier node, its Pick infoset a one-node span: updated for walker = the seat opposite
    `internal`, dropped for walker = `internal`"""
    keep = []
    got = DM.solve(FLOP_ENTRY, 0, DM.Blueprint(), 0, 4, keep=keep, **KW)
    s = keep[0]
    assert got["status"] == DM.OK and got["frontiers"] > 4 and got["rollouts"] == got["frontiers"] * 32
    external = 1 - FLOP_ENTRY.internal
    picks = {}
    for t, tree in enumerate(s.trees):
        for n in tree:
            if n.frontier is not None:
                assert s.turn(n) == ON.CHANCE and n.info is None and len(n.kids) == 1  # `randomly` kept one Pick
                child = n.kids[0]
                assert child.phase == "I" and child.info[0] == DM.PICK and child.info[3] == DRAW and s.turn(child) == external
                assert len(child.kids) == (4 if t % 2 == external else 1)
                assert all(k.phase == "E" and not k.kids and (k.k, k.j) == (child.edge, k.edge) for k in child.kids)
                picks[(t, child.info)] = child.index
    spans = {(t, info): (walker, span, head_turn) for t, walker, info, span, head_turn in s.spans}
    assert picks and all(spans[key][1] == [index] and spans[key][2] == external for key, index in picks.items())
    assert not any(len(span) > 1 and info[0] == DM.PICK for _, _, info, span, _ in s.spans), "no multi-node Pick span"
    assert {t % 2 for t, _ in picks} == {0, 1}
    # a Pick row exists exactly for the infosets met with the external seat walking
    local_picks = {info for info in s.profile.local if info[0] == DM.PICK}
    assert local_picks == {info for t, info in picks if t % 2 == external} and local_picks
    row = next(r for r in got["rows"] if r[0] == DM.PICK)
    assert row[1] == 4 and (row[5]["visits"][:4] >= 1).all() and not row[5][4:].view(np.uint8).any()


def test_origin_street_values_chance_leaves_by_stored_payoffs():
    """adapt_leaf as written: no frontier, no rollout; a chance leaf is worth cum_payoff(first choice) of its parent's infoset — the
    blueprint's until that infoset has a local row, the local row's afterwards"""
    keep, bp = [], Fixed()
    got = DM.solve(FLOP_ENTRY, None, bp, 0, 6, keep=keep, **KW)
    s = keep[0]
    assert got["status"] == DM.OK and got["frontiers"] == 0 and got["rollouts"] == 0 and not s.frontier_log
    sources = set()
    for t, tree in enumerate(s.trees):
        for n in tree:
            if n.phase == "D" and DM.inner_turn(n.game) == ON.CHANCE:
                assert not n.kids and n.frontier is None  # a leaf
                info = n.parent.info
                assert info[0] == DM.GAME
                sources.add("local" if info in s.profile.local else "blueprint")
    assert "local" in sources  # after six iterations the parents of chance leaves have rows of their own
    # both sources, read through terminal_value on a fresh solve: before and after the parent's infoset is updated
    fresh = DM.Solve(FLOP_ENTRY, 1, bp, 0, **KW)
    nodes, _ = fresh.build(0)
    leaf = next(n for n in nodes if n.phase == "D" and DM.inner_turn(n.game) == ON.CHANCE and fresh.turn(n.parent) == 0)
    info = leaf.parent.info
    assert fresh.terminal_value(leaf, 0) == fresh.terminal_value(leaf, 1) == bp.enc(info[1:])["payoff"][0]  # not negated for the other seat
    fresh.step()
    assert info in fresh.profile.local
    stored = fresh.profile.local[info][0]["payoff"]
    assert fresh.terminal_value(leaf, 0) == stored and fresh.profile.local[info][0]["visits"] == 1


@pytest.mark.parametrize("origin", [0, None])
def test_refined_is_a_distribution(origin):
    got = DM.solve(FLOP_ENTRY, origin, DM.Blueprint(), 0, 5, **KW)
    n = got["n_actions"]
    assert got["status"] == DM.OK and n == 7 and (got["refined"][:n] > 0).all() and not got["refined"][n:].any()
    assert abs(float(got["refined"].astype(np.float64).sum()) - 1.0) < 1e-6
    assert got["iterations"] == 5 and got["n_rows"] == len(got["rows"]) > 0
    keys = [(r[0], r[2], r[3], r[4]) for r in got["rows"]]  # (kind, past, present, choices)
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


def same(a, b):
    scalars = all(np.atleast_1d(a[k]).tobytes() == np.atleast_1d(b[k]).tobytes() for k in a if k != "rows")
    return scalars and len(a["rows"]) == len(b["rows"]) and all(x[:5] == y[:5] and x[5].tobytes() == y[5].tobytes() for x, y in zip(a["rows"], b["rows"]))


def test_determinism_in_seed_and_id():
    bp = DM.Blueprint()
    kw = dict(KW, first_id=0)
    base = DM.solve(FLOP_ENTRY, 0, bp, 7, 3, **kw)
    assert same(base, DM.solve(FLOP_ENTRY, 0, bp, 7, 3, **kw))
    assert same(base, DM.solve(FLOP_ENTRY, 0, bp, 3, 3, **dict(kw, first_id=4)))  # first_id + i decides, not the split
    assert not same(base, DM.solve(FLOP_ENTRY, 0, bp, 8, 3, **kw))
    assert not same(base, DM.solve(FLOP_ENTRY, 0, bp, 7, 3, **dict(kw, seed=12)))


def test_a_short_solve_is_the_start_of_a_long_one():
    bp = DM.Blueprint()
    long = DM.Solve(FLOP_ENTRY, 0, bp, 2, **KW)
    for t in range(1, 5):
        long.step()
        assert same(long.harvest(), DM.solve(FLOP_ENTRY, 0, bp, 2, t, **KW)), t


def test_malformed_entries_and_origins():
    bp = DM.Blueprint()
    assert DM.solve(Frontier((cards(51, 50), cards(50, 25)), 0), 0, bp)["status"] == FM.CARDS  # one deck: the holes are distinct
    assert DM.solve(Frontier((cards(51, 50), cards(51, 50)), 0), 0, bp)["status"] == FM.CARDS  # the reference's `wipe` state
    assert DM.solve(FLOP_ENTRY, 4, bp)["status"] == FM.SEAT and DM.solve(FLOP_ENTRY, -2, bp)["status"] == FM.SEAT
    for entry in (Frontier(HOLES, 0, edges=[OPEN2, CALL], prefix=[OPEN2, CALL]), Frontier(HOLES, 0, edges=[OPEN2, FOLD])):
        got = DM.solve(entry, None, bp, 0, 3, **KW)  # a chance entry under adapt_leaf, a terminal entry: valid, nothing to solve
        assert got["status"] == DM.OK and got["n_actions"] == 0 and got["infosets"] == 0 and got["nodes"] == 3 and not got["refined"].any()


def test_a_profile_that_outgrows_its_rows_ends_the_solve_with_a_status(monkeypatch):
    """RP_DEPTH_ROWS: a zero result and no rows, whatever the solve had got to"""
    monkeypatch.setattr(DM, "MAX_ROWS", 5)
    got = DM.solve(FLOP_ENTRY, 0, DM.Blueprint(), 0, 6, **KW)
    assert got["status"] == DM.ROWS and got["n_rows"] == 0 and not got["rows"] and got["iterations"] == 0 and got["nodes"] == 0
    assert not got["refined"].any() and got["n_actions"] == 0
    assert DM.solve(FLOP_ENTRY, 0, DM.Blueprint(), 0, 1, **KW)["status"] == DM.OK  # one iteration fits five rows

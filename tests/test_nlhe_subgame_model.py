"""Pins the model of the safe subgame re-solve (tests/nlhe_subgame_model.py) without a GPU: a river entry worked by hand over two worlds
and its harvest over all four, the tree of RP_NLHE_SUBGAME_ORIGIN_NONE (the rest of the entry street, chance leaves valued by stored
payoffs, no rollout), the deals against nlhe_world_model.restrict with 4 096 deals, the prefix property, and — with one world holding
every hole and the deal forced to the entry's own — the depth model's solve under the tag."""
import ctypes as C

import numpy as np
import pytest

import nlhe_depth_model as DM
import nlhe_policy_model as PM
import nlhe_range_model as RM
import nlhe_rollout_model as FM
import nlhe_subgame_model as SM
import nlhe_world_model as WM
import oracle_nlhe as ON
from robopoker_amd.nlhe import Frontier, Recall

F = np.float32
EPS = PM.EPSILON
OPEN2, POT = ON.Open(2), ON.RaiseOdds(1, 1)
DRAW, FOLD, CHECK, CALL, SHOVE = ON.E_DRAW, ON.E_FOLD, ON.E_CHECK, ON.E_CALL, ON.E_SHOVE


def cards(*cs):
    return sum(1 << c for c in cs)


HOLES, FLOP, TURN, RIVER = (cards(51, 50), cards(12, 25)), cards(3, 17, 30), cards(44), cards(9)
FLOP_ENTRY = Frontier(HOLES, 0, [FLOP], [OPEN2, CALL, DRAW])
FLOP_RECALL = Recall(0, HOLES[0], [FLOP], [OPEN2, CALL, DRAW])
KW = dict(rollouts=2, bp_epoch=3, prior=64.0, seed=11, first_id=5)
SPREAD = ((np.arange(RM.MAX_HOLES) % 4).astype(np.uint8), np.array([0.4, 0.3, 0.2, 0.1], F))  # every world has members and weight


class Empty:
    """a blueprint without a row"""

    def enc(self, key):
        return None

    get = enc


def payoff(g, seat):
    out = C.c_float()
    assert ON.lib().ora_nlhe_payoff(C.byref(g), seat, C.byref(out)) == 0
    return F(out.value)


def after(g, edge):
    o, g = ON.lib(), FM._copy(g)
    assert o.ora_nlhe_apply(C.byref(g), C.byref(o.ora_nlhe_snap(C.byref(g), o.ora_nlhe_actionize(C.byref(g), edge, 0)))) == 0
    return g


def same(a, b):
    scalars = all(np.atleast_1d(a[k]).tobytes() == np.atleast_1d(b[k]).tobytes() for k in a if k not in ("rows", "deals"))
    return scalars and a["deals"] == b["deals"] and len(a["rows"]) == len(b["rows"]) and \
        all(x[:6] == y[:6] and x[6].tobytes() == y[6].tobytes() for x, y in zip(a["rows"], b["rows"]))


def test_the_candidate_index_is_the_hand_iterators():
    free = SM.free_cards(HOLES[0], FLOP)
    holes = RM.hand_iterator(HOLES[0] | FLOP)
    assert len(holes) == 47 * 46 // 2 and all(SM.candidate(free, int(h)) == j for j, h in enumerate(holes))


def test_the_edge_order_is_the_derived_ord():
    """Fold < Check < Call < Open(n) < Raise(Odds) < Shove; Odds as pairs: 1/1 sorts before 1/2 before 1/4 before 2/1"""
    codes = sorted(range(1, 20), key=SM.edge_order)
    assert codes[:4] == [DRAW, FOLD, CHECK, CALL] and codes[4:8] == [ON.Open(n) for n in (2, 3, 4, 5)] and codes[-1] == SHOVE
    pairs = [ON.RAISES[c - 10] for c in codes[8:18]]
    assert pairs == sorted(ON.RAISES) == [(1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (2, 3), (3, 1), (3, 2), (3, 4), (5, 4)]
    # and it is not slot order: a flop infoset's slots run raises (grid order), Shove, Call / Check, Fold
    slots = [int(e) for e in PM.edges(FM.key_at(FM.frontier_game(FLOP_ENTRY), [], 0)[2])[:7]]
    assert slots != sorted(slots, key=SM.edge_order) and slots[-1] == CHECK and SHOVE in slots


def by_hand(g, seed, tree):
    """one walker-0 iteration of the three-leaf river tree (tests/test_nlhe_depth_model.py works it the same way) on an empty blueprint:
    -> (regret of Shove, Call, Fold after the update, ev)"""
    v_fold, v_call = payoff(after(g, FOLD), 0), payoff(after(g, CALL), 0)
    u = FM.u01(FM.node_hash(seed, DM.DRAW_EPOCH, tree, 3))  # seat 1 answers the shove: weights EPSILON each, q = 1/2 each
    pick = SHOVE if F(0.5) > u else FOLD
    sigma = F(EPS / F(100.0)) if pick == SHOVE else F(F(100.0) / F(100.0))
    v_shove = F(F(1.0) * F(F(sigma / F(0.5)) * payoff(after(after(g, SHOVE), pick), 0)))
    rd = F(F(EPS + F(50.0)) + F(100.0))
    ev = F(F(F(F(0.0) + F(F(EPS / rd) * v_shove)) + F(F(F(50.0) / rd) * v_call)) + F(F(F(100.0) / rd) * v_fold))
    return [F(EPS + F(v_shove - ev)), F(F(50.0) + F(v_call - ev)), F(F(100.0) + F(v_fold - ev))], ev


def test_a_river_entry_by_hand_over_two_worlds():
    """Seat 0 faces a pot bet on the river (tests/test_nlhe_depth_model.py's tree: Shove, Call, Fold; a shove leaves seat 1 Shove or
    Fold).  The belief has two worlds of weight; the seed is one whose iterations 0, 1, 2 draw worlds a, a, b: seat 0 walks in
    iterations 0 and 2, so its infoset gets one row in each world, each from ITS iteration's deal — the showdown is against the hole
    dealt — and worlds 2 and 3, never drawn, answer the harvest from the blueprint."""
    entry = Frontier((HOLES[0], 0), 0, [FLOP, TURN, RIVER], [OPEN2, CALL, DRAW, CHECK, CHECK, DRAW, CHECK, CHECK, DRAW, POT], [POT], stacks=(20, 20))
    hole_world = (np.arange(RM.MAX_HOLES) % 2).astype(np.uint8)
    weights = np.array([0.5, 0.5, 0.0, 0.0], F)
    first_id = 5
    worlds = lambda seed: [WM.draw_world(weights, FM.u01(WM.Deal(seed, first_id * SM.MAX_ITERATIONS + t).draw(0))) for t in range(3)]  # noqa: E731
    seed = next(s for s in range(100) if worlds(s)[0] == worlds(s)[1] != worlds(s)[2])
    keep = []
    got = SM.solve(entry, hole_world, weights, None, Empty(), 0, 3, keep=keep, rollouts=2, bp_epoch=3, prior=64.0, seed=seed, first_id=first_id)
    s = keep[0]
    a, _, b = worlds(seed)
    assert got["status"] == SM.OK and [d[1] for d in s.deals] == [a, a, b] and got["drawn"] == [[a, a, b].count(w) for w in range(4)]
    assert got["frontiers"] == 0 and got["iterations"] == 3 and got["fallbacks"] == 0 and got["attempts"] == sum(d[2] for d in s.deals)
    free = SM.free_cards(HOLES[0], FLOP | TURN | RIVER)
    assert len(free) == 45 and all(hole_world[SM.candidate(free, d[0])] == d[1] for d in s.deals)  # each hole is of its world
    choices = s.trees[0][0].info[3]
    assert list(PM.edges(choices)[:3]) == [SHOVE, CALL, FOLD] and s.trees[0][0].info[4] == a and s.trees[2][0].info[4] == b
    third = F(EPS / F(F(EPS + EPS) + EPS))
    warm = F(F(F(third * F(64.0)) * F(65.0)) / F(2.0))
    policy = PM.distribution("iterated", [EPS, F(50.0), F(100.0)] + [0] * 6, 3)[:3]
    root = {}
    for t, world in ((0, a), (2, b)):
        regret, ev = by_hand(FM.frontier_game(SM.with_hole(entry, s.deals[t][0])), seed, first_id * SM.MAX_ITERATIONS + t)
        row = next(r for r in got["rows"] if r[0] == world and r[1] == SM.GAME and r[3] == ON.path_pack([POT]) and r[5] == choices)
        assert row[2] == 3 and [x.tobytes() for x in row[6]["regret"][:3]] == [x.tobytes() for x in regret], (t, world)
        want_weight = [np.fmax(F(warm + F(p * F(t))), EPS) for p in policy]  # LinearWeight at epoch t on the warm start
        assert [x.tobytes() for x in row[6]["weight"][:3]] == [x.tobytes() for x in want_weight]
        assert (row[6]["payoff"][:3] == ev).all() and (row[6]["visits"][:3] == 1).all() and not row[6][3:].view(np.uint8).any()
        root[world] = regret
    assert [r[0] for r in got["rows"]] == sorted(r[0] for r in got["rows"]) and {r[0] for r in got["rows"]} == {a, b}
    # the harvest: worlds a and b from their rows, 2 and 3 — never drawn — from the (empty) blueprint's defaults
    per_world = [root.get(w, [EPS, F(50.0), F(100.0)]) for w in range(4)]
    refined = [F(0.0)] * 3
    for w in range(4):
        p = PM.distribution("iterated", list(per_world[w]) + [0] * 6, 3)
        refined = [F(refined[x] + F(p[x] / F(4.0))) for x in range(3)]
    assert [x.tobytes() for x in got["refined"][:3]] == [x.tobytes() for x in refined] and not got["refined"][3:].any()
    assert list(got["visits"][:3]) == [2, 2, 2]  # one visit in each of the two worlds, none in the blueprint
    regret = F(0.0)
    for x in (2, 1, 0):  # Fold < Call < Shove: the BTreeMap's order, the reverse of the slots'
        for w in range(4):
            regret = F(regret + np.fmax(per_world[w][x], F(0.0)))
    assert got["regret"].tobytes() == regret.tobytes()
    assert got["n_actions"] == 3 and got["past"] == ON.path_pack([POT]) and got["choices"] == choices


def test_origin_none_ends_at_stored_payoff_leaves_and_plays_no_rollout():
    keep, bp = [], DM.Blueprint()
    got = SM.solve(FLOP_ENTRY, *SPREAD, None, bp, 0, 8, keep=keep, **KW)
    s = keep[0]
    assert got["status"] == SM.OK and got["frontiers"] == 0 and got["rollouts"] == 0 and not s.frontier_log and got["n_rows"] > 2
    assert same(got, SM.solve(FLOP_ENTRY, *SPREAD, SM.ORIGIN_NONE, bp, 0, 8, **KW))  # None and the constant are one origin
    leaves = 0
    for t, tree in enumerate(s.trees):
        assert all(DM.street(n.game) == 1 for n in tree)  # the rest of the entry street, not "to the terminals"
        for n in tree:
            assert n.info is None or n.info[4] == s.deals[t][1]  # every infoset of tree t carries world t
            if n.phase == "D" and DM.inner_turn(n.game) == ON.CHANCE:
                assert not n.kids and n.frontier is None and n.parent.info[0] == SM.GAME
                leaves += 1
    assert leaves > 8
    # a chance leaf reads the stored payoff of its parent's infoset IN THE TREE'S WORLD: the blueprint's until that world has a row
    fresh = SM.Solve(FLOP_ENTRY, *SPREAD, None, DM.Blueprint(dense=True), 0, **KW)
    fresh.step()
    nodes = fresh.trees[0]
    leaf = next(n for n in nodes if n.phase == "D" and DM.inner_turn(n.game) == ON.CHANCE and fresh.turn(n.parent) == 0)
    info = leaf.parent.info
    assert info in fresh.profile.local and fresh.terminal_value(leaf, 0) == fresh.profile.local[info][0]["payoff"]
    other = info[:4] + ((info[4] + 1) % 4,)
    assert other not in fresh.profile.local
    assert fresh.profile.frontier_payoff(other) == fresh.bp.enc(info[1:4])["payoff"][0] != fresh.profile.local[info][0]["payoff"]


def test_with_origin_plays_the_continuation_game_from_the_dealt_hole():
    keep = []
    got = SM.solve(FLOP_ENTRY, *SPREAD, 0, DM.Blueprint(), 0, 4, keep=keep, **KW)
    s = keep[0]
    assert got["status"] == SM.OK and got["frontiers"] > 4 and got["rollouts"] == got["frontiers"] * 32 and len(s.frontier_log) == got["frontiers"]
    dealt = {d[0] for d in s.deals}
    assert {record.holes[1] for record, _, _ in s.frontier_log} == dealt and HOLES[1] not in dealt
    assert all(record.holes[0] == HOLES[0] for record, _, _ in s.frontier_log)
    assert any(r[1] == SM.PICK for r in got["rows"]) and any(r[1] == SM.GAME for r in got["rows"])
    keys = [(r[0], r[1], r[3], r[4], r[5]) for r in got["rows"]]  # (world, kind, past, present, choices)
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


def test_the_other_seats_hole_is_not_read():
    bp = DM.Blueprint()
    want = SM.solve(FLOP_ENTRY, *SPREAD, 0, bp, 0, 3, **KW)
    for other in (0, HOLES[0], cards(3, 17), 1 << 60):  # nothing, internal's own cards, two of the board, no card at all
        assert same(want, SM.solve(Frontier((HOLES[0], other), 0, [FLOP], [OPEN2, CALL, DRAW]), *SPREAD, 0, bp, 0, 3, **KW))
    assert SM.solve(Frontier((cards(51), HOLES[1]), 0, [FLOP], [OPEN2, CALL, DRAW]), *SPREAD, 0, bp, 0, 3, **KW)["status"] == FM.CARDS


@pytest.mark.parametrize("origin", [None, 0])
def test_a_short_solve_is_the_start_of_a_long_one(origin):
    bp = DM.Blueprint()
    long = SM.Solve(FLOP_ENTRY, *SPREAD, origin, bp, 2, **KW)
    for t in range(1, 5):
        long.step()
        short = SM.solve(FLOP_ENTRY, *SPREAD, origin, bp, 2, t, **KW)
        assert same(long.harvest(), short) and sum(short["drawn"]) == t, t
    assert same(long.harvest(), SM.solve(FLOP_ENTRY, *SPREAD, origin, bp, 0, 4, **dict(KW, first_id=7)))  # first_id + i decides


def test_every_deal_is_restricts_deal_t_of_4096():
    """a real belief (the opponent's range of an untrained table, cut into four worlds): the solve's deals are what
    nlhe_world_model.restrict answers for the recall of `internal` with deals = 4096 — which buckets every attempted hole again"""
    bel = WM.belief(FLOP_RECALL, {})
    assert bel["status"] == RM.OK and all((bel["hole_world"][: bel["count"]] == w).any() for w in range(4))
    keep = []
    got = SM.solve(FLOP_ENTRY, bel["hole_world"], bel["weights"], None, DM.Blueprint(), 3, 6, keep=keep, **KW)
    holes, worlds, attempts = WM.restrict(FLOP_RECALL, bel, 3, SM.MAX_ITERATIONS, None, KW["seed"], KW["first_id"])
    assert got["status"] == SM.OK and got["deals"] == [(int(holes[t]), int(worlds[t]), int(attempts[t])) for t in range(6)]
    assert got["drawn"] == [int((worlds[:6] == w).sum()) for w in range(4)] and got["attempts"] == int(attempts[:6].sum())


def test_one_world_and_the_entrys_own_hole_is_the_depth_solve():
    """the tree draws share epoch 2 and the id with the depth solve, so with the deal forced to the entry's own hole and one world
    holding every hole the trees, the frontier payoffs and the profile are nlhe_depth_model's; the rows carry the tag, and the
    harvest still averages four worlds, three of which have no row"""
    for origin, depth_origin in ((0, 0), (None, None)):  # depth origin None = the entry's street: no frontier either
        bp = DM.Blueprint()
        keep = []
        got = SM.solve(FLOP_ENTRY, *SM.one_world(FLOP_ENTRY, 2), origin, bp, 1, 5, keep=keep, force=HOLES[1], **KW)
        want = DM.solve(FLOP_ENTRY, depth_origin, bp, 1, 5, **KW)
        assert got["status"] == want["status"] == SM.OK and got["drawn"] == [0, 0, 5, 0] and got["attempts"] == 0
        for f in ("nodes", "infosets", "frontiers", "rollouts", "n_rows", "iterations", "past", "present", "choices", "n_actions"):
            assert got[f] == want[f], f
        assert got["sum_regret"].tobytes() == want["sum_regret"].tobytes()
        assert [r[:1] + r[1:6] for r in got["rows"]] == [(2,) + r[:5] for r in want["rows"]]
        assert all(x[6].tobytes() == y[5].tobytes() for x, y in zip(got["rows"], want["rows"]))
        n = want["n_actions"]
        info = (SM.GAME, want["past"], want["present"], want["choices"], 2)
        assert np.asarray(keep[0].profile.iterated(info), F).tobytes() == want["refined"][:n].tobytes()
        assert got["refined"].tobytes() != want["refined"].tobytes()  # three worlds answer from the blueprint


def test_malformed_beliefs_entries_and_origins():
    bp = DM.Blueprint()
    hw, wt = SPREAD
    for bad in (np.nan, -0.5, np.inf):
        assert SM.solve(FLOP_ENTRY, hw, np.array([0.5, bad, 0.25, 0.25], F), None, bp)["status"] == FM.CARDS
    assert SM.solve(FLOP_ENTRY, hw, np.zeros(4, F), None, bp, 0, 2)["drawn"] == [2, 0, 0, 0]  # all zero: world 0
    assert SM.solve(FLOP_ENTRY, hw, wt, 4, bp)["status"] == FM.SEAT and SM.solve(FLOP_ENTRY, hw, wt, -2, bp)["status"] == FM.SEAT
    assert SM.solve(FLOP_ENTRY, hw, wt, 127, bp)["status"] == FM.SEAT  # the depth solve's ORIGIN_ENTRY is no origin here
    assert SM.solve(Frontier(HOLES, 0, [FLOP], [OPEN2, CALL, DRAW, 25]), hw, wt, 4, bp)["status"] == FM.EDGE  # the record's status first
    assert SM.solve(Frontier(HOLES, 0, [FLOP], [OPEN2, CALL, DRAW]), hw, np.array([np.nan] * 4, F), 9, bp)["status"] == FM.SEAT  # then the origin's
    # a byte that is no world reads as none: 77 everywhere leaves no member, every deal takes the fallback
    got = SM.solve(FLOP_ENTRY, np.full(RM.MAX_HOLES, 77, np.uint8), wt, None, bp, 0, 2, **KW)
    assert got["status"] == SM.OK and got["fallbacks"] == 2 and got["attempts"] == 2 * SM.MAX_REJECTIONS
    for entry in (Frontier(HOLES, 0, edges=[OPEN2, CALL], prefix=[OPEN2, CALL]), Frontier(HOLES, 0, edges=[OPEN2, FOLD])):
        got = SM.solve(entry, hw, wt, None, bp, 0, 3, **KW)  # a chance entry, a terminal entry: valid, nothing to solve
        assert got["status"] == SM.OK and got["n_actions"] == 0 and got["infosets"] == 0 and got["nodes"] == 3 and not got["refined"].any()
        assert sum(got["drawn"]) == 3


def test_a_profile_that_outgrows_its_rows_ends_the_solve_with_a_status(monkeypatch):
    monkeypatch.setattr(SM, "MAX_ROWS", 5)
    got = SM.solve(FLOP_ENTRY, *SPREAD, 0, DM.Blueprint(), 0, 6, **KW)
    assert got["status"] == DM.ROWS and got["n_rows"] == 0 and not got["rows"] and got["iterations"] == 0 and got["drawn"] == [0] * 4
    assert not got["deals"] and got["attempts"] == 0
    assert DM.MAX_ROWS == 512  # the depth model's own cap is back where it was

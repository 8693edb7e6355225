"""tests/mccfr_depth_model.py on its own (no device): the known answer of the continuation game as the reference builds it, and
DepthSolver against the W = 1 entry form of SubGameSolver::with_origin.

The known answer.  Seat 0 chooses between a terminal paying it c and a depth-1 chance state whose continuation matrix (row = seat
0's k, column = seat 1's j) is [[2, -1], [-1, 0]]; D = 2, origin 0, a zero blueprint.  The frontier node stays a chance node, so k is
drawn uniformly and never learnt: seat 1 answers the column of the smaller MEAN, and the frontier is worth min_j mean_k M[k][j] =
min(0.5, -0.5) = -0.5 to seat 0 — not the matrix game's value -0.25.  So at c = -0.4 the refined policy moves to the terminal (slot
0), at c = -0.6 to the frontier (slot 1): a solver that learnt k would keep the frontier in both.

ITERATIONS is the smallest power of two at which the model's refined probability of the right slot is at least 0.75 for the eight
seeds 0 .. 7 in a row, in both cases: measured 2^10 (c = -0.4 still answers 0.48 under seed 0 at 2^9; c = -0.6 needs 2^7)."""
import numpy as np
import pytest

import mccfr_depth_cases as C
import mccfr_depth_model as D
import mccfr_subgame_model as M
import oracle
from robopoker_amd import Game, games

ITERATIONS = 1 << 10
SEEDS = range(8)


@pytest.mark.parametrize("c,right", [(-0.4, 0), (-0.6, 1)])
def test_known_answer_the_frontier_is_worth_the_smaller_column_mean(c, right):
    _, table, fr, entry, rows = C.known_answer(c)
    bp = M.Blueprint(table, rows)
    for seed in SEEDS:
        r = D.solve(table, bp, fr, entry, 0, iterations=ITERATIONS, seed=seed)
        assert r["status"] == M.OK and r["n_actions"] == 2 and r["frontiers"] > 0
        print(f"c = {c}, seed {seed}: refined {r['refined'][:2]}")
        assert r["refined"][right] >= 0.75, (c, seed, r["refined"][:2])
        picks = [row for row in r["rows"] if row[1] == D.PICK]
        assert len(picks) == 1 and picks[0][:4] == (0, D.PICK, 2, 0)


def test_origin_none_and_an_origin_at_the_frontiers_depth_grow_no_frontier():
    _, table, fr, entry, rows = C.known_answer(-0.4)
    bp = M.Blueprint(table, rows)
    for origin in (D.ORIGIN_NONE, 1, 200):
        r = D.solve(table, bp, fr, entry, origin, iterations=16, seed=3)
        base = M.solve(table, bp, entry, iterations=16, seed=3)
        assert r["frontiers"] == 0 and all(row[1] == D.GAME for row in r["rows"])
        assert [(w, n, i, e.tobytes()) for w, _, n, i, e in r["rows"]] == [(w, n, i, e.tobytes()) for w, n, i, e in base["rows"]]
        assert r["refined"].tobytes() == base["refined"].tobytes() and r["nodes"] == base["nodes"]
    assert D.solve(table, bp, fr, entry, D.ORIGIN_ENTRY, iterations=16, seed=3)["frontiers"] > 0  # depth[observed] = 0


@pytest.fixture(scope="module")
def leduc():
    g = Game("leduc")
    ora = oracle.OracleSolver(g, "floored", "linear", "external", batch=1, seed=0).solve(1 << 12)
    t = M.Table(g.table)
    return g, t, M.Blueprint(t, ora.export())


@pytest.mark.parametrize("leaves", C.LEAVES)
def test_depth_solver_is_the_one_world_entry_form(leduc, leaves):
    """DepthSolver::new(source, prefix, internal, entry) stepped and harvested on its own equals the entry {observed = entry, external =
    1 - internal, n_candidates = 0, n_worlds = 1, weights = {1}} at ORIGIN_ENTRY: the same trees, the same rows under world 0, the
    same harvest; `fallbacks` counts every iteration"""
    g, t, bp = leduc
    fr = C.builtin_frontiers(g, leaves)
    for holes, prefix, internal in (((4, 1), (), 0), ((0, 3), (0,), 1), ((2, 5), (1,), 0), ((1, 4), (0, 1), 0), ((0, 2), (0, 0), 1)):
        entry = games.depth_entry(g, holes, prefix, internal)[0]
        kept = []
        got = D.solve(t, bp, fr, entry, D.ORIGIN_ENTRY, index=2, iterations=40, seed=9, first_id=1, keep=kept)
        alone = D.DepthSolver(t, bp, fr, games.play(g, holes, prefix), internal, index=2, seed=9, first_id=1)
        for _ in range(40):
            alone.step()
        assert got["status"] == M.OK and got["fallbacks"] == 40 and list(got["drawn"]) == [40, 0, 0, 0]
        assert (got["nodes"], got["infosets"], got["frontiers"]) == (alone.nodes, alone.infosets, alone.n_frontiers)
        rows = alone.exported(lambda key: 0)
        assert [(r[:4], r[4].tobytes()) for r in rows] == [(r[:4], r[4].tobytes()) for r in got["rows"]]
        assert F32(alone.profile.sum_regret()) == F32(got["sum_regret"])
        if t.decision(int(entry["observed"])):
            info = t.info[int(entry["observed"])]
            refined, visits, regret = alone.harvest(info, [int(x) for x in entry["harvest_order"]])
            n = t.actions[info]
            assert [F32(x) for x in refined] == [F32(x) for x in got["refined"][:n]] and visits == list(got["visits"][:n])
            assert F32(regret) == F32(got["regret"])
            assert got["frontiers"] > 0  # origin = depth(entry) = 0 in round 1: the board deal is a frontier
        else:  # entered at the board deal, origin = depth(entry) = 1: no frontier, a leaf, nothing to update
            assert got["n_actions"] == 0 and got["n_rows"] == 0 and got["frontiers"] == 0 and got["nodes"] == 40
            at0 = D.solve(t, bp, fr, entry, 0, iterations=40, seed=9)  # the same state under origin 0 is a frontier entry state
            assert at0["n_actions"] == 0 and at0["frontiers"] == 40 and at0["n_rows"] == 1 and at0["rows"][0][:2] == (0, D.PICK)


def F32(x):
    return int(np.float32(x).view(np.uint32))


def test_pick_infosets_are_shared_across_seat_ones_card(leduc):
    """frontier states that differ only in seat 1's card carry one Pick infoset: two worlds' rows differ in the world tag alone"""
    g, t, bp = leduc
    fr = C.builtin_frontiers(g, 2)
    a, b = games.play(g, (0, 2), (0, 0)), games.play(g, (0, 5), (0, 0))
    assert t.turn[a] == t.turn[b] == M.CHANCE and a != b and fr.pick_info[a] == fr.pick_info[b] < fr.n_pick
    assert fr.pick_info[games.play(g, (2, 5), (0, 0))] != fr.pick_info[a]  # seat 0's rank differs


def test_inconsistent_tables_are_a_status_and_a_tree_of_frontiers_overflows():
    g, table, fr, entry = C.overflowing()
    bp = M.Blueprint(table, np.zeros(table.n_infos * table.A, M.ENC))
    assert D.solve(table, bp, fr, entry, 0, iterations=2)["status"] == M.TREE  # iteration 1: walker = external keeps everything
    assert D.solve(table, bp, fr, entry, 0, iterations=1)["status"] == M.OK
    assert D.solve(table, bp, fr, entry, D.ORIGIN_NONE, iterations=2)["status"] == M.OK
    fr.n_pick = 3
    assert D.solve(table, bp, fr, entry, 0, iterations=64)["status"] == D.FRONTIER

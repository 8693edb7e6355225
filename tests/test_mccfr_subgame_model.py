"""tests/mccfr_subgame_model.py on its own (no device): the partition on hand-worked posteriors, the restrict rule's three arms, the
reference's restrict_produces_valid_deals, the model's prefix property, and the reference's subgame thresholds (kuhn/src/solver.rs:
294-517, leduc/src/solver.rs:165-285) on a blueprint from the CPU oracle solver, which equals the device bit for bit in ORDERED mode.

The model runs about 5 000 Kuhn iterations a second, so one Kuhn case (reach-conditioned: both of its assertions) and one Leduc case
(the root) run the reference's full 2^16 iterations against its thresholds; the other entries run 2^12 iterations WITHOUT a threshold
(they check that the solve runs and stays finite).  The device test (test_gpu_mccfr_subgame.py) runs every entry at full length."""
import numpy as np
import pytest

import game_tables
import mccfr_subgame_cases as K
import mccfr_subgame_model as M
import oracle
from robopoker_amd import Game, _lib, games

F = np.float32
NONE = _lib.RP_WORLD_NONE


def test_partition_by_hand():
    # W = 1: one world takes everything
    mapping, w = M.partition([(0, F(1)), (1, F(2)), (2, F(2))], 1)
    assert mapping == {0: 0, 1: 0, 2: 0} and list(w) == [1, 0, 0, 0]
    # W = 2, ties keep ascending secret: sorted (1, 2) (2, 2) (0, 1); segment 2.5; 2 < 2.5; 4 >= 2.5 closes world 0 at 4/5
    mapping, w = M.partition([(0, F(1)), (1, F(2)), (2, F(2))], 2)
    assert mapping == {1: 0, 2: 0, 0: 1} and list(w) == [F(4) / F(5), F(1) / F(5), 0, 0]
    # W = 4 with three entries: at most one advance per entry, so world 3 is never reached and keeps weight 0
    mapping, w = M.partition([(0, F(4)), (1, F(1)), (2, F(1))], 4)
    assert mapping == {0: 0, 1: 1, 2: 2} and list(w) == [F(4) / F(6), F(1) / F(6), F(1) / F(6), 0]
    # W = 4, one dominant entry: 8 >= 2.5 advances once (an `if`, not a `while`), the rest fills world 1
    mapping, w = M.partition([(3, F(8)), (5, F(1)), (9, F(1))], 4)
    assert mapping == {3: 0, 5: 1, 9: 2} and list(w) == [F(0.8), F(0.1), F(0.1), 0]
    # total <= 0, no entry at all included: world 0 and uniform weights over W
    for entries in ([], [(2, F(0)), (7, F(0))]):
        mapping, w = M.partition(entries, 4)
        assert mapping == {s: 0 for s, _ in entries} and list(w) == [0.25] * 4
    mapping, w = M.partition([(2, F(0))], 2)
    assert list(w) == [0.5, 0.5, 0, 0]


@pytest.fixture(scope="module")
def kuhn():
    g = Game("kuhn")
    ora = oracle.OracleSolver(g, "floored", "linear", "external", batch=1, seed=0).solve(1 << 18)
    t = M.Table(g.table)
    return g, t, M.Blueprint(t, ora.export())


@pytest.fixture(scope="module")
def leduc():
    g = Game("leduc")
    ora = oracle.OracleSolver(g, "floored", "linear", "external", batch=1, seed=0).solve(1 << 18)
    t = M.Table(g.table)
    return g, t, M.Blueprint(t, ora.export())


def entry_of(game, table, bp, holes, prefix, external, reach, W=2):
    prior, entry = games.subgame_entry(game, holes, prefix, external, reach, n_worlds=W)
    b = M.belief(table, bp, prior[0])
    assert b["status"] == M.OK
    return K.with_belief(entry[0], b), b


def test_restrict_three_arms(kuhn):
    g, t, bp = kuhn
    e, b = entry_of(g, t, bp, (4, 1), (), 1, False)  # seat 0 holds K0; J J Q Q K: J, Q in world 0, K in world 1
    assert list(b["world_of"][:3]) == [0, 0, 1]
    s = M.Solve(t, bp, e)
    assert s.restrict(0) == (games.play(g, (4, 0), ()), True) and s.restrict(1) == (games.play(g, (4, 5), ()), True)
    none = e.copy()
    none["world_of"] = NONE  # no members at all: every candidate is remembered, the first wins whatever the world
    assert M.Solve(t, bp, none).restrict(1) == (games.play(g, (4, 0), ()), True)
    lone = e.copy()
    lone["world_of"][:3] = 0  # world 1 has weight but no member: the observed state, counted as a fallback
    assert M.Solve(t, bp, lone).restrict(1) == (int(e["observed"]), False)
    empty = e.copy()
    empty["n_candidates"] = 0
    assert M.Solve(t, bp, empty).restrict(0) == (int(e["observed"]), False)


@pytest.mark.parametrize("name", ["kuhn", "leduc"])
def test_restrict_produces_valid_deals(name, request):
    """kuhn/src/solver.rs:443-453, leduc/src/solver.rs:234-244, for every deal instead of a random one"""
    g, t, bp = request.getfixturevalue(name)
    for holes in [(a, b) for a in range(6) for b in range(6) if a != b]:
        e, _ = entry_of(g, t, bp, holes, (), 1, False)
        s = M.Solve(t, bp, e)
        for w in range(2):
            state, chosen = s.restrict(w)
            assert chosen
            dealt = [c for c in range(6) if c != holes[0] and games.play(g, (holes[0], c), ()) == state]
            assert len(dealt) == 1 and dealt[0] != holes[0]


def test_prefix_property_and_every_case_runs(kuhn, leduc):
    for g, t, bp in (kuhn, leduc):
        for label, e in K.builtin_cases(g, t, bp):
            long = M.Solve(t, bp, e, 3, seed=5)
            short = M.Solve(t, bp, e, 3, seed=5)
            for _ in range(24):
                long.step()
            for _ in range(9):
                short.step()
            assert [[n.state for n in tr] for tr in short.trees] == [[n.state for n in tr] for tr in long.trees[:9]], label
            nine = M.solve(t, bp, e, index=3, iterations=9, seed=5)
            assert nine["status"] == M.OK and nine["n_rows"] == short.harvest()["n_rows"], label
            assert int(nine["drawn"].sum()) == 9 and np.isfinite(nine["sum_regret"]), label
    big = game_tables.game("chance16_mid")
    t = M.Table(big.table)
    ora = oracle.OracleSolver(big, "floored", "linear", "external", batch=1, seed=3).solve(2000)
    bp = M.Blueprint(t, ora.export())
    for label, e in K.custom_cases(t, bp):
        r = M.solve(t, bp, e, iterations=9)
        assert r["status"] == M.OK and r["n_actions"] in (2, 3), label
    for status, e in K.malformed(K.custom_cases(t, bp)[1][1], t):  # the W = 2 variant
        assert M.solve(t, bp, e, iterations=2)["status"] == status


def kuhn_call(g, t, bp, result, name):
    return M.averaged_policy(t, bp, result["rows"], g.info_id(name), 2)[K.CALL]


def test_known_answer_kuhn_reach_conditioned_full_length(kuhn):
    """kuhn/src/solver.rs:462-517 at 2^16 iterations: sum_regret < 0.01, K|XB Call > 0.90"""
    g, t, bp = kuhn
    e, _ = entry_of(g, t, bp, (0, 4), (K.CHECK, K.BET), 1, True)
    r = M.solve(t, bp, e, iterations=1 << 16, seed=1)
    assert r["status"] == M.OK and r["sum_regret"] < 0.01, r["sum_regret"]
    assert kuhn_call(g, t, bp, r, "K|XB") > 0.90


def test_known_answer_leduc_root_full_length(leduc):
    """leduc/src/solver.rs:165-183 at 2^16 iterations: sum_regret < 0.5"""
    g, t, bp = leduc
    e, _ = entry_of(g, t, bp, (2, 5), (), 1, False)
    r = M.solve(t, bp, e, iterations=1 << 16, seed=1)
    assert r["status"] == M.OK and r["sum_regret"] < 0.5, r["sum_regret"]


@pytest.mark.parametrize("name,prefix,external,reach", [("kuhn", (), 1, False), ("kuhn", (K.CHECK,), 0, False), ("kuhn", (K.BET,), 0, False),
                                                        ("leduc", (K.CHECK,), 0, False), ("leduc", (K.BET,), 0, False),
                                                        ("leduc", (K.CHECK, K.BET), 1, True)])
def test_other_entries_run_shortened_without_a_threshold(name, prefix, external, reach, request):
    g, t, bp = request.getfixturevalue(name)
    e, _ = entry_of(g, t, bp, (3, 4), prefix, external, reach)
    r = M.solve(t, bp, e, iterations=1 << 12, seed=1)
    assert r["status"] == M.OK and np.isfinite(r["sum_regret"]) and int(r["drawn"].sum()) == 1 << 12

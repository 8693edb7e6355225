"""The skeleton traversal reads the game through packed rows — one row of infoset ids, payoffs and draw keys per sequence of
chance outcomes (DevGame::rows, RowLayout in csrc/traverse_static.hpp) — and its infosets through one 32-byte row each
(DevInfoTab::row2).  RP_TRAV_NO_FLAT=1 keeps the child-record chain, one dependent load per node: an independent way to the same
words.  Both are stepped side by side against the CPU oracle; tables and counters must be equal bit for bit after every step.
"""
import numpy as np
import pytest

import oracle
from robopoker_amd import Game
from robopoker_amd.mccfr import Solver

pytestmark = pytest.mark.gpu

STEPS = 6  # both walkers three times; long enough for the sampling weights and the keep masks to leave their defaults


def assert_tables_equal(a: np.ndarray, b: np.ndarray, what: str):
    for f in ("visits", "regret", "weight", "payoff"):
        if a[f].dtype.kind == "f":
            assert not np.isnan(a[f]).any(), f"{what}: NaN in {f}"
        assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), f"{what}: {f} differs bitwise"


# one ragged chunk (three full wavefronts and 8 lanes of a fourth); five full 256-tree chunks and a ragged sixth
@pytest.mark.parametrize("batch", [200, 1357])
@pytest.mark.parametrize("mode", ["ordered", "composed"])
@pytest.mark.parametrize("rng", ["counter", "reference"])
@pytest.mark.parametrize("sampling", ["external", "prunable", "pluribus"])
@pytest.mark.parametrize("game", ["kuhn", "leduc"])
def test_packed_rows_and_child_records_equal_the_oracle(gpu, monkeypatch, game, sampling, rng, mode, batch):
    g = Game(game)
    hp = oracle.default_hyper()
    hp.prune_warmup, hp.prune_threshold, hp.prune_explore = 2, -0.05, 0.1  # pruning bites from the third step on
    rows = Solver(g, "linear", "linear", sampling, batch=batch, seed=61, hyper=hp)
    monkeypatch.setenv("RP_TRAV_NO_FLAT", "1")
    kids = Solver(g, "linear", "linear", sampling, batch=batch, seed=61, hyper=hp)
    monkeypatch.delenv("RP_TRAV_NO_FLAT")
    ora = oracle.OracleSolver(g, "linear", "linear", sampling, batch=batch, seed=61, hyper=hp)
    assert rows.kernel_variant() == kids.kernel_variant() == "static"
    assert rows.traversal_rows_bytes() > 0 and kids.traversal_rows_bytes() == 0
    if rng == "reference":
        for s in (rows, kids, ora):
            s.set_rng("reference")
    if mode == "composed":
        rows.set_update_mode("composed")
        kids.set_update_mode("composed")
    for step in range(STEPS):
        rows.step()
        kids.step()
        if mode == "composed":
            ora.step_world(1)
        else:
            ora.step()
        want = ora.export()
        assert_tables_equal(rows.export(), want, f"packed rows, step {step}")
        assert_tables_equal(kids.export(), want, f"child records, step {step}")
        assert rows.counters() == kids.counters() == ora.counters(), f"step {step}"


@pytest.mark.parametrize("game", ["kuhn", "leduc"])
def test_rows_fit_the_vector_l1(gpu, game):
    # Leduc: 64-byte rows for round 1 (one per pair of private cards) and for each of the three round-2 sub-trees (one per pair and
    # board card), 16-byte rows for the second deal — under the 32 KB of a CU's vector L1, where the 16-byte records (56 KB) were not
    s = Solver(Game(game), "floored", "linear", "external", batch=64, seed=1)
    assert 0 < s.traversal_rows_bytes() <= 32 * 1024 and s.traversal_rows_bytes() % 128 == 0

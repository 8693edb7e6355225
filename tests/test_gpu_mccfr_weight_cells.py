"""The fused traversal (k_traverse_maps_static) keeps three values per Decisions in LDS — two regret deltas and the payoff — and no
weight delta: every entry of an infoset's list carries the same two sigmas, the ones of the infoset's row the traversal itself read, and
the epoch is uniform over the grid, so the lanes of the two weight cells compute weight_delta(W, row2[info][c & 1], t) once, before the
chain, and touch with that register (csrc/traverse_static.hpp).  Same operand, same operation, same order: nothing may move a bit.
Tables and counters against the CPU oracle's blocked composition after every step.

Batches: one lane; one wavefront; a chunk less one, exactly one, one more; two chunks and a ragged third of one tree (513).
Four steps: each walker twice, the second time on sigmas that are no longer the initial ones.
Schedules, so that every weight rule meets both chain loops: (floored, constant | linear | quadratic) run the unit-discount loop,
(floored, exponential) the general loop through the weight discount 0.9999, (linear, linear) the general loop through the regret discount.
All three samplings — the pruned ones keep the edge masks behind the three cells, where a wrong offset shows once the masks bite (from the
second step on) — and both draw kinds.  Two shards with an exchange window of three: the epoch changes between the local steps of a
window while the sigmas do not.
"""
import numpy as np
import pytest

import oracle
from robopoker_amd import Game
from robopoker_amd.mccfr import Solver

pytestmark = pytest.mark.gpu

STEPS = 4
SEED = 41
BATCHES = [1, 64, 255, 256, 257, 513]
SCHEDULES = [("floored", "constant"), ("floored", "linear"), ("floored", "quadratic"), ("floored", "exponential"), ("linear", "linear")]
SAMPLINGS = ["external", "prunable", "pluribus"]
DRAWS = ["counter", "reference"]


def hyper():
    hp = oracle.default_hyper()
    hp.prune_warmup, hp.prune_threshold, hp.prune_explore = 1, -0.05, 0.1  # pruning bites from the second step on
    return hp


def assert_tables_equal(a: np.ndarray, b: np.ndarray, what: str):
    for f in ("visits", "regret", "weight", "payoff"):
        if a[f].dtype.kind == "f":
            assert not np.isnan(a[f]).any(), f"{what}: NaN in {f}"
        assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), f"{what}: {f} differs bitwise"


def composed(game, regret, weight, sampling, batch, draws="counter", seed=SEED):
    s = Solver(Game(game), regret, weight, sampling, batch=batch, seed=seed, hyper=hyper())
    s.set_update_mode("composed")
    if draws == "reference":
        s.set_rng("reference")
    assert s.kernel_variant() == "static"
    return s


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("draws", DRAWS)
@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("regret,weight", SCHEDULES)
@pytest.mark.parametrize("game", ["kuhn", "leduc"])
def test_fused_step_equals_the_oracle(gpu, game, regret, weight, sampling, draws, batch):
    s = composed(game, regret, weight, sampling, batch, draws)
    ora = oracle.OracleSolver(Game(game), regret, weight, sampling, batch=batch, seed=SEED, hyper=hyper())
    if draws == "reference":
        ora.set_rng("reference")
    what = f"{game} {regret}/{weight}/{sampling} {draws} batch {batch}"
    for step in range(STEPS):
        s.step()
        ora.step_world(1)
        assert_tables_equal(s.export(), ora.export(), f"{what}, step {step}")
        assert s.counters() == ora.counters(), f"{what}, step {step}: (nodes, infos)"
    assert s.epoch == ora.epoch == STEPS
    s.close()


def test_fused_equals_unfused_array_for_array(gpu, monkeypatch):
    # RP_TRAV_UNFUSED is read at creation: the same step as k_traverse_static + k_chunk_maps, whose lists still carry the weight deltas
    # of every entry.  Quadratic weight: the delta is two multiplications away from the sigma
    fused = composed("leduc", "floored", "quadratic", "pluribus", 513)
    monkeypatch.setenv("RP_TRAV_UNFUSED", "1")
    unfused = composed("leduc", "floored", "quadratic", "pluribus", 513)
    monkeypatch.delenv("RP_TRAV_UNFUSED")
    for step in range(STEPS):
        fused.step()
        unfused.step()
        a, b = fused.export(), unfused.export()
        assert a.dtype == b.dtype
        for f in a.dtype.names:
            assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), f"step {step}: {f}"
        assert fused.counters() == unfused.counters(), f"step {step}"
    fused.close()
    unfused.close()


def test_two_shards_with_an_exchange_window_of_three(gpu):
    # two handles play the ranks of a world of 2; each composes three local steps into one summary before the exchange: within a window
    # the epoch (and with it the weight delta of an unchanged sigma) moves from local step to local step
    import torch

    g, world, window, batch = Game("leduc"), 2, 3, 513
    devs = [Solver(g, "floored", "linear", "external", batch=batch, seed=12) for _ in range(world)]
    for r, d in enumerate(devs):
        d.set_shard(r, world)
    n = devs[0].summary_bytes()
    gathered = torch.zeros(n * world, dtype=torch.uint8, device="cuda")
    ora = oracle.OracleSolver(g, "floored", "linear", "external", batch=batch, seed=12)
    for w in range(2):
        for r, d in enumerate(devs):
            for k in range(window):
                d.window_local(gathered.data_ptr() + r * n, k == 0)
            d.sync()
        for d in devs:
            d.window_apply(gathered.data_ptr(), world)
            d.sync()
        ora.window_world(world, window)
        for d in devs:
            assert_tables_equal(d.export(), ora.export(), f"window {w}")
    assert devs[0].epoch == 2 * window == ora.epoch
    for d in devs:
        d.close()

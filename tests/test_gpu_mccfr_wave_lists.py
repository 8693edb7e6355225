"""The fused traversal (k_traverse_maps_static) builds the per-infoset lists of its 256-tree chunk in wavefront 0 alone: lane r reads
the bitmap row of the walker's infoset of rank r, the lists' bases are a scan across the lanes, the places of the (infoset, cell) tasks
come from one ballot per length class, and `order` holds the walker's infosets only (csrc/traverse_static.hpp).  Nothing of it may move
a bit: tables and counters against the CPU oracle's blocked composition after every step.

Batches: one lane; a wavefront less one, exactly one, one more; a chunk less one, exactly one, one more; five chunks and a ragged
sixth (1357 trees).  Four steps: each walker twice, the second time on tables that are no longer the initial ones.
Games: kuhn (6 infosets per player: most lanes of the wavefront idle) and leduc (60).  Schedules: (floored, linear) runs the
unit-discount chain loop, (linear, linear) the general one.  All three samplings (the pruned ones carry the edge masks in the lists)
and both draw kinds.
"""
import numpy as np
import pytest

import oracle
from robopoker_amd import Game
from robopoker_amd.mccfr import Solver

pytestmark = pytest.mark.gpu

STEPS = 4
SEED = 97
BATCHES = [1, 63, 64, 65, 255, 256, 257, 1357]
SCHEDULES = [("floored", "linear"), ("linear", "linear")]
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


@pytest.mark.parametrize("regret,weight", SCHEDULES)
@pytest.mark.parametrize("game,batch", [("kuhn", 257), ("leduc", 1357)])
def test_two_shards_with_an_exchange_window_of_three(gpu, game, batch, regret, weight):
    # two handles play the ranks of a world of 2; each composes three local steps into one summary before the exchange
    import torch

    g, world, window = Game(game), 2, 3
    devs = [Solver(g, regret, weight, "external", batch=batch, seed=12) for _ in range(world)]
    for r, d in enumerate(devs):
        d.set_shard(r, world)
    n = devs[0].summary_bytes()
    gathered = torch.zeros(n * world, dtype=torch.uint8, device="cuda")
    ora = oracle.OracleSolver(g, regret, weight, "external", batch=batch, seed=12)
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


@pytest.mark.parametrize("regret,weight,sampling", [("floored", "linear", "external"), ("linear", "linear", "pluribus")])
def test_the_same_run_twice_gives_the_same_tables(gpu, regret, weight, sampling):
    runs = []
    for _ in range(2):
        s = composed("leduc", regret, weight, sampling, 1357)
        trace = []
        for _ in range(STEPS):
            s.step()
            trace.append((s.export(), s.counters()))
        runs.append(trace)
        s.close()
    for step, ((a, ca), (b, cb)) in enumerate(zip(*runs)):
        assert_tables_equal(a, b, f"step {step}")
        assert ca == cb, f"step {step}"


@pytest.mark.parametrize("regret,weight,sampling", [("floored", "linear", "external"), ("linear", "linear", "pluribus")])
@pytest.mark.parametrize("game", ["kuhn", "leduc"])
def test_fused_equals_unfused_array_for_array(gpu, monkeypatch, game, regret, weight, sampling):
    # RP_TRAV_UNFUSED is read at creation: the same step as k_traverse_static + k_chunk_maps, which build their lists for all infosets
    fused = composed(game, regret, weight, sampling, 1357)
    monkeypatch.setenv("RP_TRAV_UNFUSED", "1")
    unfused = composed(game, regret, weight, sampling, 1357)
    monkeypatch.delenv("RP_TRAV_UNFUSED")
    for step in range(STEPS):
        fused.step()
        unfused.step()
        a, b = fused.export(), unfused.export()
        assert a.dtype == b.dtype
        for f in a.dtype.names:
            assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), f"{game} {sampling}, step {step}: {f}"
        assert fused.counters() == unfused.counters(), f"{game} {sampling}, step {step}"
    fused.close()
    unfused.close()

"""The chain phase of the fused composed step (csrc/traverse_static.hpp k_traverse_maps_static): when the regret and the weight
discount are both exactly 1.0 the five chains of an infoset's list — two regret cells, two weight cells, the payoff sum — run side by
side in one loop whose touch has no multiplication (map_touch_unit_unless); any other schedule keeps the general touch and the separate
payoff pass.  Neither may change a bit: tables and counters against the CPU oracle's blocked composition after every step, and the
callers that reach the fused step by other roads (shards, exchange windows, a resumed solver).

Batches: one lane; a ragged chunk; exactly one chunk; one tree in a second chunk; several chunks.  Six steps: each walker three times,
and the epoch changes the weight delta from step to step.
"""
import functools

import numpy as np
import pytest

import oracle
from robopoker_amd import Game
from robopoker_amd.mccfr import Solver

pytestmark = pytest.mark.gpu

STEPS = 6
SEED = 101
BATCHES = [1, 255, 256, 257, 1357]
SAMPLINGS = ["external", "prunable", "pluribus"]
# (regret, weight): both discounts 1.0 (the one-loop unit touch) three times; a weight, a regret, both discounts other than 1.0 (general)
SCHEDULES = [("floored", "linear"), ("summed", "constant"), ("floored", "quadratic"), ("summed", "exponential"), ("linear", "linear"),
             ("linear", "exponential")]


def hyper():
    hp = oracle.default_hyper()
    hp.prune_warmup, hp.prune_threshold, hp.prune_explore = 2, -0.05, 0.1  # pruning bites from the third step on
    return hp


def assert_tables_equal(a: np.ndarray, b: np.ndarray, what: str):
    for f in ("visits", "regret", "weight", "payoff"):
        if a[f].dtype.kind == "f":
            assert not np.isnan(a[f]).any(), f"{what}: NaN in {f}"
        assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), f"{what}: {f} differs bitwise"


@functools.lru_cache(maxsize=None)
def oracle_trace(game, regret, weight, sampling, rng, batch):
    """(table, counters) of the oracle's blocked composition after each step"""
    ora = oracle.OracleSolver(Game(game), regret, weight, sampling, batch=batch, seed=SEED, hyper=hyper())
    if rng == "reference":
        ora.set_rng("reference")
    out = []
    for _ in range(STEPS):
        ora.step_world(1)
        out.append((ora.export(), ora.counters()))
    return out


def run_against_oracle(game, regret, weight, sampling, rng, batch):
    s = Solver(Game(game), regret, weight, sampling, batch=batch, seed=SEED, hyper=hyper())
    assert s.kernel_variant() == "static"
    if rng == "reference":
        s.set_rng("reference")
    s.set_update_mode("composed")
    what = f"{game} {regret}/{weight}/{sampling}/{rng} batch {batch}"
    for step, (want, counters) in enumerate(oracle_trace(game, regret, weight, sampling, rng, batch)):
        s.step()
        assert_tables_equal(s.export(), want, f"{what}, step {step}")
        assert s.counters() == counters, f"{what}, step {step}: (nodes, infos)"
    s.close()


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("regret,weight", SCHEDULES)
@pytest.mark.parametrize("game", ["kuhn", "leduc"])
def test_composed_step_equals_the_oracle(gpu, game, regret, weight, sampling, batch):
    run_against_oracle(game, regret, weight, sampling, "counter", batch)


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("game", ["kuhn", "leduc"])
def test_composed_step_equals_the_oracle_reference_draws(gpu, game, sampling, batch):
    run_against_oracle(game, "floored", "linear", sampling, "reference", batch)


# ---- the other callers of the fused step --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regret,weight", [("floored", "linear"), ("summed", "exponential")])
def test_two_shards_on_one_gpu_match_the_world_model(gpu, regret, weight):
    import torch

    g, B, world = Game("leduc"), 257, 2
    devs = [Solver(g, regret, weight, "external", batch=B, seed=33) for _ in range(world)]
    for r, d in enumerate(devs):
        d.set_shard(r, world)
    n = devs[0].summary_bytes()
    gathered = torch.zeros(n * world, dtype=torch.uint8, device="cuda")
    ora = oracle.OracleSolver(g, regret, weight, "external", batch=B, seed=33)
    for step in range(4):
        for r, d in enumerate(devs):
            d.step_local(gathered.data_ptr() + r * n)
            d.sync()
        for d in devs:
            d.step_apply(gathered.data_ptr(), world)
            d.sync()
        ora.step_world(world)
        for d in devs:
            assert_tables_equal(d.export(), ora.export(), f"shards, step {step}")
    for d in devs:
        d.close()


@pytest.mark.parametrize("regret,weight", [("floored", "linear"), ("summed", "exponential")])
def test_exchange_window_of_three_matches_the_world_model(gpu, regret, weight):
    # inside a window the table is frozen while the epoch advances: the weight delta still changes from step to step
    import torch

    g, B, world, window = Game("leduc"), 257, 2, 3
    devs = [Solver(g, regret, weight, "external", batch=B, seed=12) for _ in range(world)]
    for r, d in enumerate(devs):
        d.set_shard(r, world)
    n = devs[0].summary_bytes()
    gathered = torch.zeros(n * world, dtype=torch.uint8, device="cuda")
    ora = oracle.OracleSolver(g, regret, weight, "external", batch=B, seed=12)
    for w in range(3):
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
    assert devs[0].epoch == 3 * window == ora.epoch
    for d in devs:
        d.close()


def test_a_resumed_solver_takes_the_same_step(gpu):
    g = Game("leduc")
    a = Solver(g, "floored", "linear", "external", batch=1357, seed=SEED)
    a.set_update_mode("composed")
    for _ in range(5):
        a.step()
    rows, epoch = a.export(), a.epoch
    b = Solver(g, "floored", "linear", "external", batch=1357, seed=SEED)
    b.set_update_mode("composed")
    b.load_rows(rows, epoch)
    a.step()
    b.step()
    assert b.epoch == a.epoch == epoch + 1
    assert_tables_equal(b.export(), a.export(), "resumed")
    a.close()
    b.close()

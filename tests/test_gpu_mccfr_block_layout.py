"""The block maps of the composed update are chunk-major and compacted by walker (csrc/mccfr_kernels.hpp bmap_index): row `block`
holds, for each of the walker's infosets in rank order, 2A cell maps and one {payoff sum, count} slot.  Three kernels write the rows
(k_traverse_maps_static in both chain-phase branches, k_chunk_maps, k_block_maps) and k_combine2 folds them, lane = (infoset, slot),
first inside groups of RP_FOLD_GROUP = 64 blocks, then — the last group of an infoset tile to arrive — across the groups.  None of it may
move a bit: tables and counters against the CPU oracle's blocked composition after every step.

Batches: one lane; a ragged chunk; exactly one chunk; one tree in a second chunk; exactly one full group (64 chunks); a second group
that holds one block of one tree; four groups with the last one ragged (194 chunks, the last of 44 trees), where the order of the
second-level fold matters.  Four steps: each walker twice.
Games and writers: kuhn (one infoset tile) and leduc (two tiles) through the fused kernel, leduc through k_chunk_maps, leduc_wide
(616 infosets, many tiles) through k_chunk_maps<., CM_PASSES> and, with the per-infoset slot map forced, through k_block_maps.
"""
import functools

import numpy as np
import pytest

import oracle
from robopoker_amd import Game
from robopoker_amd.mccfr import Solver

pytestmark = pytest.mark.gpu

STEPS = 4
SEED = 211
BATCHES = [1, 255, 256, 257, 16384, 16385, 49452]
# unit discounts (the one-loop chain phase of the fused kernel); general touch with pruned edges; a weight discount other than 1.0
SCHEDULES = [("floored", "linear", "external"), ("linear", "quadratic", "pluribus"), ("summed", "exponential", "external")]
# (game, environment of the solver's creation, whether the step sorts its Decisions first).  All five traverse with the skeleton
# kernels (kernel_variant "static"); the sort (k_count / k_scan / k_compact) runs on the slot-map path alone, the one that ends in
# k_block_maps, and its launch count tells that path from the others.  The library does not report whether the traversal and the
# block maps were one kernel or two: the fused kernel exists for at most 256 infosets (kuhn 12, leduc 120, not leduc_wide's 616) and
# RP_TRAV_UNFUSED is read at creation; tests/test_gpu_mccfr.py compares the two spellings directly.
PATHS = {
    "kuhn-fused": ("kuhn", {}, False),
    "leduc-fused": ("leduc", {}, False),
    "leduc-chunk_maps": ("leduc", {"RP_TRAV_UNFUSED": "1"}, False),
    "wide-chunk_maps": ("leduc_wide", {}, False),
    "wide-block_maps": ("leduc_wide", {"RP_MCCFR_SLOTMAP": "1"}, True),
}


def hyper():
    hp = oracle.default_hyper()
    hp.prune_warmup, hp.prune_threshold, hp.prune_explore = 1, -0.05, 0.1  # pruning bites from the second step on
    return hp


def assert_tables_equal(a: np.ndarray, b: np.ndarray, what: str):
    for f in ("visits", "regret", "weight", "payoff"):
        if a[f].dtype.kind == "f":
            assert not np.isnan(a[f]).any(), f"{what}: NaN in {f}"
        assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), f"{what}: {f} differs bitwise"


@functools.lru_cache(maxsize=None)
def oracle_trace(game, regret, weight, sampling, batch):
    """(table, counters) of the oracle's blocked composition after each step; shared by the writers of one game and read-only"""
    ora = oracle.OracleSolver(Game(game), regret, weight, sampling, batch=batch, seed=SEED, hyper=hyper())
    out = []
    for _ in range(STEPS):
        ora.step_world(1)
        table = ora.export()
        table.setflags(write=False)
        out.append((table, ora.counters()))
    return out


def make_solver(monkeypatch, game, env, regret, weight, sampling, batch, seed=SEED):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = Solver(Game(game), regret, weight, sampling, batch=batch, seed=seed, hyper=hyper())
    for k in env:
        monkeypatch.delenv(k)
    s.set_update_mode("composed")
    s.profile(True)  # counts the launches of the sort (kernel_time): which writer of the block maps ran
    return s


def assert_path_taken(s, sorts, steps, what):
    assert s.kernel_variant() == "static", what
    assert s.kernel_time("compact")[1] == (steps if sorts else 0), f"{what}: launches of the sort"


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("regret,weight,sampling", SCHEDULES)
@pytest.mark.parametrize("path", list(PATHS))
def test_composed_step_equals_the_oracle(gpu, monkeypatch, path, regret, weight, sampling, batch):
    game, env, sorts = PATHS[path]
    s = make_solver(monkeypatch, game, env, regret, weight, sampling, batch)
    what = f"{path} {regret}/{weight}/{sampling} batch {batch}"
    for step, (want, counters) in enumerate(oracle_trace(game, regret, weight, sampling, batch)):
        s.step()
        assert_tables_equal(s.export(), want, f"{what}, step {step}")
        assert s.counters() == counters, f"{what}, step {step}: (nodes, infos)"
    assert_path_taken(s, sorts, STEPS, what)
    s.close()


# ---- the summary blob (k_combine2<false>): identity cells and zero sums for the other player's infosets -----------------------------
@pytest.mark.parametrize("regret,weight", [("floored", "linear"), ("summed", "exponential")])
@pytest.mark.parametrize("game,batch", [("kuhn", 257), ("leduc", 16385)])
def test_two_shards_on_one_gpu_match_the_world_model(gpu, game, batch, regret, weight):
    import torch

    g, world = Game(game), 2
    devs = [Solver(g, regret, weight, "external", batch=batch, seed=33) for _ in range(world)]
    for r, d in enumerate(devs):
        d.set_shard(r, world)
    n = devs[0].summary_bytes()
    gathered = torch.zeros(n * world, dtype=torch.uint8, device="cuda")
    ora = oracle.OracleSolver(g, regret, weight, "external", batch=batch, seed=33)
    for step in range(STEPS):
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
    import torch

    g, B, world, window = Game("leduc"), 16385, 2, 3
    devs = [Solver(g, regret, weight, "external", batch=B, seed=12) for _ in range(world)]
    for r, d in enumerate(devs):
        d.set_shard(r, world)
    n = devs[0].summary_bytes()
    gathered = torch.zeros(n * world, dtype=torch.uint8, device="cuda")
    ora = oracle.OracleSolver(g, regret, weight, "external", batch=B, seed=12)
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


# ---- which group arrives last is timing; what the tables hold is not -----------------------------------------------------------------
@pytest.mark.parametrize("path", ["leduc-fused", "wide-chunk_maps"])
def test_the_same_run_twice_gives_the_same_tables(gpu, monkeypatch, path):
    game, env, _ = PATHS[path]
    runs = []
    for _ in range(2):
        s = make_solver(monkeypatch, game, env, "floored", "linear", "external", 49452)
        trace = []
        for _ in range(STEPS):
            s.step()
            trace.append(s.export())
        runs.append(trace)
        s.close()
    for step, (a, b) in enumerate(zip(*runs)):
        assert_tables_equal(a, b, f"{path}, step {step}")

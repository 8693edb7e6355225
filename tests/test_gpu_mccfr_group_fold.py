"""The second level of the composed update's fold, the group maps of a batch composed in group order, runs in one of two places
(csrc/mccfr_update.hpp): inside k_combine2, by the last workgroup of an infoset tile to arrive ("fused"), or in a launch of its own,
k_fold_groups after k_combine2<false, false>, one workgroup per infoset that stages the infoset's group maps in LDS, slab by slab
("split").  The host chooses by the number of groups (Solver.fold_variant()); RP_FOLD_SPLIT=1 / 0, read at creation, forces the split
from one group upward / never.  Neither place may move a bit: the association is the oracle's, a left fold from the identity in block
order inside a group, then in group order.

Batches against the oracle: one block; a full block; two blocks in one group; exactly one group (64 blocks of 256 trees); a second group
of one tree; four groups with a ragged last group and block.  Three steps: both walkers, and a σ row re-derived by the fold and read by
the next traversal of the same walker.  Split against fused: 257 groups (more groups than the workgroup has lanes, so a lane stages
several slots of a slab) and 513 groups (one more than the 512 groups a slab holds with two actions: FG_SLOTS / (2A + 1) = 2 560 / 5).
"""
import functools

import numpy as np
import pytest

import oracle
from robopoker_amd import Game
from robopoker_amd.mccfr import Solver

pytestmark = pytest.mark.gpu

STEPS = 3
SEED = 977
BATCHES = [1, 256, 257, 16384, 16385, 49452]
# unit discounts; pruned sampling with a general regret touch; a weight discount other than 1.0
SCHEDULES = [("floored", "linear", "external"), ("linear", "quadratic", "pluribus"), ("summed", "exponential", "external")]
SPLIT, FUSED = {"RP_FOLD_SPLIT": "1"}, {"RP_FOLD_SPLIT": "0"}


def hyper():
    hp = oracle.default_hyper()
    hp.prune_warmup, hp.prune_threshold, hp.prune_explore = 1, -0.05, 0.1  # pruning bites from the second step on
    return hp


def assert_tables_equal(a: np.ndarray, b: np.ndarray, what: str):
    for f in ("visits", "regret", "weight", "payoff"):
        if a[f].dtype.kind == "f":
            assert not np.isnan(a[f]).any(), f"{what}: NaN in {f}"
        assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), f"{what}: {f} differs bitwise"


def make_solver(monkeypatch, env, game, regret, weight, sampling, batch, seed=SEED):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = Solver(Game(game), regret, weight, sampling, batch=batch, seed=seed, hyper=hyper())
    for k in env:
        monkeypatch.delenv(k)
    s.set_update_mode("composed")
    assert s.fold_variant() == ("split" if env is SPLIT else "fused")
    return s


@functools.lru_cache(maxsize=None)
def oracle_trace(game, regret, weight, sampling, batch):
    """(table, counters) of the oracle's blocked composition after each step; read-only"""
    ora = oracle.OracleSolver(Game(game), regret, weight, sampling, batch=batch, seed=SEED, hyper=hyper())
    out = []
    for _ in range(STEPS):
        ora.step_world(1)
        table = ora.export()
        table.setflags(write=False)
        out.append((table, ora.counters()))
    return out


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("regret,weight,sampling", SCHEDULES)
@pytest.mark.parametrize("game", ["kuhn", "leduc"])
def test_split_fold_equals_the_oracle(gpu, monkeypatch, game, regret, weight, sampling, batch):
    s = make_solver(monkeypatch, SPLIT, game, regret, weight, sampling, batch)
    what = f"{game} {regret}/{weight}/{sampling} batch {batch}"
    for step, (want, counters) in enumerate(oracle_trace(game, regret, weight, sampling, batch)):
        s.step()
        assert_tables_equal(s.export(), want, f"{what}, step {step}")
        assert s.counters() == counters, f"{what}, step {step}: (nodes, infos)"
    s.close()


# ---- many groups: the GPU's two folds against each other ---------------------------------------------------------------------------
@pytest.mark.parametrize("game,batch", [("kuhn", 4210944), ("leduc", 4210944), ("leduc", 8388609)])
def test_split_equals_fused_at_many_groups(gpu, monkeypatch, game, batch):
    runs = []
    for env in (SPLIT, FUSED):
        s = make_solver(monkeypatch, env, game, "linear", "exponential", "external", batch)
        trace = []
        for _ in range(2):
            s.step()
            trace.append((s.export(), s.counters()))
        runs.append(trace)
        s.close()
    for step, ((a, ca), (b, cb)) in enumerate(zip(*runs)):
        assert_tables_equal(a, b, f"{game} batch {batch}, step {step}")
        assert ca == cb, f"{game} batch {batch}, step {step}: (nodes, infos)"
        assert a["visits"].sum() > 0


# ---- the summary blob (k_fold_groups<false>): two shards, an exchange window of three ----------------------------------------------
def windows_of_two_shards(monkeypatch, env, regret, weight, batch, windows=2, window=3):
    """the shards' tables and the gathered blob after each exchange window"""
    import torch

    world = 2
    devs = [make_solver(monkeypatch, env, "leduc", regret, weight, "external", batch, seed=12) for _ in range(world)]
    for r, d in enumerate(devs):
        d.set_shard(r, world)
    n = devs[0].summary_bytes()
    gathered = torch.zeros(n * world, dtype=torch.uint8, device="cuda")
    out = []
    for _ in range(windows):
        for r, d in enumerate(devs):
            for k in range(window):
                d.window_local(gathered.data_ptr() + r * n, k == 0)
            d.sync()
        blob = gathered.cpu().numpy().copy()
        for d in devs:
            d.window_apply(gathered.data_ptr(), world)
            d.sync()
        out.append(([d.export() for d in devs], blob))
    assert devs[0].epoch == windows * window
    for d in devs:
        d.close()
    return out


@pytest.mark.parametrize("regret,weight", [("floored", "linear"), ("summed", "exponential")])
def test_exchange_window_split_equals_fused_and_the_world_model(gpu, monkeypatch, regret, weight):
    batch, world, window = 49452, 2, 3
    split = windows_of_two_shards(monkeypatch, SPLIT, regret, weight, batch)
    fused = windows_of_two_shards(monkeypatch, FUSED, regret, weight, batch)
    ora = oracle.OracleSolver(Game("leduc"), regret, weight, "external", batch=batch, seed=12, hyper=hyper())
    for w, ((ts, bs), (tf, bf)) in enumerate(zip(split, fused)):
        ora.window_world(world, window)
        want = ora.export()
        assert np.array_equal(bs, bf), f"window {w}: the gathered summary blobs differ"
        for r in range(world):
            assert_tables_equal(ts[r], tf[r], f"window {w}, shard {r}: split against fused")
            assert_tables_equal(ts[r], want, f"window {w}, shard {r}: split against the oracle")


# ---- the host's own choice ---------------------------------------------------------------------------------------------------------
def test_default_choice_by_batch(gpu, monkeypatch):
    monkeypatch.delenv("RP_FOLD_SPLIT", raising=False)
    s = Solver(Game("kuhn"), "floored", "linear", "external", batch=1 << 17, seed=1)
    s.set_update_mode("composed")
    assert s.fold_variant() == "fused"  # 8 groups: one batch of the fused tail, no third launch
    s.set_batch(1 << 23)
    assert s.fold_variant() == "split"  # 512 groups
    s.set_batch(1 << 17)
    assert s.fold_variant() == "fused"
    s.close()

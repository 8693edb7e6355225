"""k_fold_groups (csrc/mccfr_update.hpp) folds a slab of group maps in one of two ways.  A `unit` slab — every non-empty cell map and
every running map carried into it has a == 1.0f, a finite b and an m that is not NaN — is compacted in LDS and folded with two
operations per map (fold_unit_ops); every other slab by fold_slots, as before.  The choice is taken per slab from the data, for all
cells of the infoset together.  Neither may move a bit: tests/test_gpu_mccfr_group_fold.py holds for both, and with its non-unit
schedules it is now the test of the general path.  Here, with the split forced (RP_FOLD_SPLIT=1):

  - against the oracle, the batches of that file with unit schedules it does not have at these sizes: Summed / Constant (m stays -inf
    through the whole chain) and Floored / Quadratic under pruned sampling (pruned regret cells are empty in whole groups: the
    compaction), and a mixed one, Summed / Exponential: regret cells qualify, weight cells do not, the infoset takes the general path;
  - split against the one-launch fold at 257 and 513 groups with unit schedules (513: the second slab holds one group, the running
    maps are carried in and its first operand composes instead of replacing);
  - the summary blob of two shards (k_fold_groups<false>) with a unit schedule;
  - a resumed table, regrets and weights far from zero;
  - payoffs near FLT_MAX, so that regret deltas overflow: slabs with non-finite operands, by bits, NaN allowed.
"""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import game_tables as GT
import oracle
from robopoker_amd import Game, _lib
from robopoker_amd.mccfr import Solver

pytestmark = pytest.mark.gpu

STEPS = 3
SEED = 977
BATCHES = [1, 256, 257, 16384, 16385, 49452]
# unit, m == -inf throughout; unit with pruned sampling; regret cells unit and weight cells not
SCHEDULES = [("summed", "constant", "external"), ("floored", "quadratic", "pluribus"), ("summed", "exponential", "external")]
UNIT = [("floored", "linear", "external"), ("summed", "constant", "external")]
SPLIT, FUSED = {"RP_FOLD_SPLIT": "1"}, {"RP_FOLD_SPLIT": "0"}
FIELDS = ("visits", "regret", "weight", "payoff")


def hyper():
    hp = oracle.default_hyper()
    hp.prune_warmup, hp.prune_threshold, hp.prune_explore = 1, -0.05, 0.1  # pruning bites from the second step on
    return hp


def assert_tables_equal(a: np.ndarray, b: np.ndarray, what: str):
    for f in FIELDS:
        if a[f].dtype.kind == "f":
            assert not np.isnan(a[f]).any(), f"{what}: NaN in {f}"
        assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), f"{what}: {f} differs bitwise"


def assert_bits_equal(a: np.ndarray, b: np.ndarray, what: str):
    """as assert_tables_equal, for tables that may hold NaN: the same bits, whatever they spell"""
    for f in FIELDS:
        diff = np.count_nonzero(a[f].view(np.uint32) != b[f].view(np.uint32))
        assert diff == 0, f"{what}: {f} differs bitwise in {diff} cells"


def make_solver(monkeypatch, env, game, regret, weight, sampling, batch, seed=SEED, hp=None):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = Solver(Game(game) if isinstance(game, str) else game, regret, weight, sampling, batch=batch, seed=seed, hyper=hp or hyper())
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
def test_unit_fold_equals_the_oracle(gpu, monkeypatch, game, regret, weight, sampling, batch):
    s = make_solver(monkeypatch, SPLIT, game, regret, weight, sampling, batch)
    what = f"{game} {regret}/{weight}/{sampling} batch {batch}"
    for step, (want, counters) in enumerate(oracle_trace(game, regret, weight, sampling, batch)):
        s.step()
        assert_tables_equal(s.export(), want, f"{what}, step {step}")
        assert s.counters() == counters, f"{what}, step {step}: (nodes, infos)"
    s.close()


# ---- many groups: the GPU's two folds against each other ---------------------------------------------------------------------------
def two_steps(monkeypatch, env, game, regret, weight, batch, prepare=None, seed=SEED, hp=None):
    s = make_solver(monkeypatch, env, game, regret, weight, "external", batch, seed=seed, hp=hp)
    if prepare:
        prepare(s)
    trace = []
    for _ in range(2):
        s.step()
        trace.append((s.export(), s.counters()))
    s.close()
    return trace


def assert_traces_equal(split, fused, what, equal=assert_tables_equal):
    for step, ((a, ca), (b, cb)) in enumerate(zip(split, fused)):
        equal(a, b, f"{what}, step {step}")
        assert ca == cb, f"{what}, step {step}: (nodes, infos)"
        assert a["visits"].sum() > 0


@pytest.mark.parametrize("regret,weight,_", UNIT, ids=[f"{r}-{w}" for r, w, _ in UNIT])
@pytest.mark.parametrize("batch", [4210944, 8388609])
def test_unit_split_equals_fused_at_many_groups(gpu, monkeypatch, batch, regret, weight, _):
    split, fused = (two_steps(monkeypatch, env, "leduc", regret, weight, batch) for env in (SPLIT, FUSED))
    assert_traces_equal(split, fused, f"leduc {regret}/{weight} batch {batch}")


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


def test_unit_exchange_window_split_equals_fused_and_the_world_model(gpu, monkeypatch):
    regret, weight, batch, world, window = "floored", "linear", 49452, 2, 3
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


# ---- a resumed table ---------------------------------------------------------------------------------------------------------------
RESUMED_BATCH = 16385  # 64 blocks of 256 trees, and a second group of one tree


@functools.lru_cache(maxsize=None)
def resumed_rows(name):
    """a table far from zero (read-only): a 3-step oracle run, its regrets and weights scaled up, a blueprint's visits in every cell"""
    g = Game(name)
    ora = oracle.OracleSolver(g, "floored", "linear", "external", batch=8192, seed=17)
    for _ in range(3):
        ora.step()
    rows = ora.export().copy().reshape(g.n_infos, g.max_actions)
    assert np.count_nonzero(rows["visits"]) > 0
    rows["regret"] *= np.float32(3.0e4)
    rows["weight"] = rows["weight"] * np.float32(1.0e6) + np.float32(1.0e3)
    for i in range(g.n_infos):
        rows["visits"][i, : g.n_actions(i)] = (1 << 24) - 1500
        rows["regret"][i, g.n_actions(i):] = 0.0
        rows["weight"][i, g.n_actions(i):] = 0.0
    rows = rows.reshape(-1)
    assert np.isfinite(rows["regret"]).all() and np.abs(rows["regret"]).max() > 1.0e4 and rows["weight"].max() > 1.0e6
    rows.setflags(write=False)
    return rows


@pytest.mark.parametrize("regret,weight,_", UNIT, ids=[f"{r}-{w}" for r, w, _ in UNIT])
@pytest.mark.parametrize("name", ["kuhn", "leduc"])
def test_unit_fold_on_a_resumed_table(gpu, monkeypatch, name, regret, weight, _):
    rows, epoch = resumed_rows(name), (1 << 24) - 2

    def prepare(s):
        s.load_rows(rows, epoch)
        assert s.epoch == epoch

    split, fused = (two_steps(monkeypatch, env, name, regret, weight, RESUMED_BATCH, prepare, seed=43) for env in (SPLIT, FUSED))
    assert_traces_equal(split, fused, f"{name} resumed {regret}/{weight}")
    ora = oracle.OracleSolver(Game(name), regret, weight, "external", batch=RESUMED_BATCH, seed=43, hyper=hyper())
    ora.load_rows(rows, epoch)
    for step, (table, counters) in enumerate(split):
        ora.step_world(1)
        assert_tables_equal(table, ora.export(), f"{name} resumed {regret}/{weight}, step {step}: split against the oracle")


# ---- operands that are not finite --------------------------------------------------------------------------------------------------
class HugePayoffGame:
    """a freshly built two-action catalogue game whose terminal payoffs are scaled towards FLT_MAX before any solver sees the table:
    the payoffs are finite, the difference of two of them is not"""

    def __init__(self, name, scale):
        why, players, plan, dr, variant = GT._SPECS[name]
        self.base = GT.TableGame(players, plan, default_regret=dr, seed=zlib.crc32(name.encode()))
        t = self.base.table
        n = t.n_terminals * t.n_players
        pay = np.array(t.payoffs[:n], dtype=np.float32) * np.float32(scale)
        assert np.isfinite(pay).all() and float(pay.max()) - float(pay.min()) > float(np.finfo(np.float32).max)
        self._payoffs = (C.c_float * n)(*pay.tolist())
        self.table = _lib.GameTable.from_buffer_copy(t)
        self.table.payoffs = self._payoffs
        self.n_infos, self.max_actions = t.n_infos, t.max_actions

    def n_actions(self, info):
        return self.base.n_actions(info)

    def player(self, info):
        return self.base.player(info)


@pytest.mark.parametrize("regret,weight,_", UNIT, ids=[f"{r}-{w}" for r, w, _ in UNIT])
def test_overflowing_regret_deltas_split_equals_fused(gpu, monkeypatch, regret, weight, _):
    g = HugePayoffGame("depth10", 1.6e38)  # payoffs are multiples of 0.25 in [-2, 2]
    assert g.max_actions == 2
    hp = oracle.default_hyper()
    split, fused = (two_steps(monkeypatch, env, g, regret, weight, RESUMED_BATCH, seed=5, hp=hp) for env in (SPLIT, FUSED))
    assert_traces_equal(split, fused, f"depth10 x 1.6e38 {regret}/{weight}", equal=assert_bits_equal)
    # the input does what the name says: the tables hold regrets that are no finite number
    assert not np.isfinite(split[-1][0]["regret"]).all()

"""GPU parity on CALLER-BUILT game tables (tests/game_tables.py): the dense MCCFR solver against the CPU oracle, bit for bit.

The built-in games never reach k_traverse_lds<false> (5..16 actions), the payoff path of n_players != 2, a walker rotation over one or
three players, a table's default_regret, 1-action infosets, a player root, or the natural fall-through to the HBM-scratch traversal.
Each game of the catalogue exists for one of these; every case first asserts the traversal kernel the game must select
(rp_mccfr_traversal_variant), which is what proves that a boundary of the LDS traversal is hit from the intended side.

Only tables rp_game_table_check accepts are handed to the device here; the refused ones are in tests/test_game_tables_custom.py.
"""
import numpy as np
import pytest

import game_tables as GT
import oracle
from mccfr_hand import chance_draw
from robopoker_amd.mccfr import Solver

pytestmark = pytest.mark.gpu

VARIANT = ("hbm", "lds")
LIMIT_PAIR = ("infos8191", "infos8192")  # 29 000 states: one configuration only
PARITY = [n for n in GT.CATALOGUE if n != "chance16_root" and n not in LIMIT_PAIR]
# (update mode, regret, weight, sampling, batch).  600 trees = more than two RP_COMPOSE_CHUNKs: several block maps per cell are folded
# Floored regret never falls below the pruning threshold (only widest_a16's negative default_regret does), so PrunableSampling bites
# under the linear schedule of the third configuration; Pluribus bites in the composed one (node counts drop by a tenth to a quarter)
CONFIGS = [("ordered", "discounted", "linear", "external", 130), ("ordered", "floored", "linear", "prunable", 130),
           ("ordered", "linear", "linear", "prunable", 130), ("composed", "linear", "quadratic", "pluribus", 600)]


def pruning_hyper():
    """the constants of test_pruned_masks_follow_from_the_table: pruning bites within a few epochs"""
    hp = oracle.default_hyper()
    hp.prune_warmup, hp.prune_threshold, hp.prune_explore = 2, -0.05, 0.3
    return hp


def assert_same_state(dev, ora, what="", counters=True):
    a, b = dev.export(), ora.export()
    for f in ("visits", "regret", "weight", "payoff"):
        if a[f].dtype.kind == "f":
            assert not np.isnan(a[f]).any(), f"NaN in {f} {what}"
        assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), f"{f} differs bitwise {what}"
    assert dev.epoch == ora.epoch, what
    if counters:
        assert dev.counters() == ora.counters(), what


def pair(g, regret, weight, sampling, batch, seed, mode="ordered", hyper=None):
    hp = hyper if hyper is not None else pruning_hyper()
    dev = Solver(g, regret, weight, sampling, batch=batch, seed=seed, hyper=hp)
    ora = oracle.OracleSolver(g, regret, weight, sampling, batch=batch, seed=seed, hyper=hp)
    if mode == "composed":
        dev.set_update_mode("composed")
    return dev, ora


def run(dev, ora, mode, steps, what):
    for s in range(steps):
        dev.step()
        if mode == "composed":
            ora.step_world(1)
        else:
            ora.step()
        assert_same_state(dev, ora, f"{what}, step {s}")


@pytest.mark.parametrize("mode,regret,weight,sampling,batch", CONFIGS, ids=[f"{c[0]}-{c[1]}-{c[3]}" for c in CONFIGS])
@pytest.mark.parametrize("name", PARITY)
def test_catalogue_tables_bit_exact_vs_oracle(gpu, name, mode, regret, weight, sampling, batch):
    g = GT.game(name)
    dev, ora = pair(g, regret, weight, sampling, batch, seed=31, mode=mode)
    assert dev.kernel_variant() == VARIANT[GT.CATALOGUE[name]["variant"]]
    run(dev, ora, mode, 5, name)
    # host-side quantities over the same tables
    assert dev.sum_regret() == ora.sum_regret()
    assert dev.exploitability() == ora.exploitability()
    for info in range(g.n_infos):
        for kind in ("iterated", "averaged", "sampling"):
            assert np.array_equal(dev.policy(info, kind).view(np.uint32), ora.policy(info, kind).view(np.uint32)), (info, kind)


def test_three_player_exploitability_and_policies_equal_the_oracle(gpu):
    # after steps of all three walkers, twice round
    g = GT.game("three_players_a5")
    dev, ora = pair(g, "linear", "linear", "external", 257, seed=8)
    run(dev, ora, "ordered", 6, "three_players_a5")
    assert np.float32(dev.exploitability()).view(np.uint32) == np.float32(ora.exploitability()).view(np.uint32)
    for info in range(g.n_infos):
        for kind in ("iterated", "averaged", "sampling"):
            got = dev.policy(info, kind)
            assert got.size == g.n_actions(info)
            assert np.array_equal(got.view(np.uint32), ora.policy(info, kind).view(np.uint32)), (info, kind)


@pytest.mark.parametrize("name", LIMIT_PAIR)
def test_the_infoset_limit_of_the_lds_traversal(gpu, name):
    # 8191 infosets are the most the LDS traversal's node word can name (13 bits); 8192 take the HBM-scratch traversal.  Both run the
    # large-game update kernels (more than 256 infosets)
    g = GT.game(name)
    dev, ora = pair(g, "floored", "linear", "external", 130, seed=31)
    assert dev.kernel_variant() == VARIANT[GT.CATALOGUE[name]["variant"]]
    run(dev, ora, "ordered", 5, name)


@pytest.mark.parametrize("name", ["three_players_a5", "widest_a16"])
def test_hbm_scratch_override_on_caller_built_tables(gpu, monkeypatch, name):
    # the generic HBM-scratch traversal forced on games that fit LDS: the same tables as the LDS traversal and the oracle
    g = GT.game(name)
    lds, ora = pair(g, "linear", "linear", "pluribus", 300, seed=77)
    monkeypatch.setenv("RP_MCCFR_HBM_SCRATCH", "1")
    hbm = Solver(g, "linear", "linear", "pluribus", batch=300, seed=77, hyper=pruning_hyper())
    monkeypatch.delenv("RP_MCCFR_HBM_SCRATCH")
    assert (lds.kernel_variant(), hbm.kernel_variant()) == ("lds", "hbm")
    for s in range(6):
        lds.step()
        hbm.step()
        ora.step()
        assert_same_state(lds, ora, f"{name} lds, step {s}")
        assert_same_state(hbm, ora, f"{name} hbm, step {s}")


@pytest.mark.parametrize("batch", [1, 63, 64, 65, 257])
def test_batch_edges_on_three_players(gpu, batch):
    # one tree, a wave less one, a wave, a wave and one, a chunk and one — over all three walkers
    dev, ora = pair(GT.game("three_players_a5"), "linear", "linear", "external", batch, seed=7)
    run(dev, ora, "ordered", 3, f"batch {batch}")


def test_three_player_shards_on_one_gpu_match_the_world_model(gpu):
    # two handles play the ranks of a world of 2 (set_shard / step_local / step_apply), the summaries exchanged by hand, against
    # ora_mccfr_step_world(2): all three walkers, the block maps compacted by walker (rank_count / rank_info with three owners)
    import torch

    g = GT.game("three_players_a5")
    B, world = 300, 2
    devs = [Solver(g, "linear", "linear", "external", batch=B, seed=33) for _ in range(world)]
    for r, d in enumerate(devs):
        d.set_shard(r, world)
    n = devs[0].summary_bytes()
    gathered = torch.zeros(n * world, dtype=torch.uint8, device="cuda")
    ora = oracle.OracleSolver(g, "linear", "linear", "external", batch=B, seed=33)
    for s in range(3):
        for r, d in enumerate(devs):
            d.step_local(gathered.data_ptr() + r * n)
            d.sync()
        for d in devs:
            d.step_apply(gathered.data_ptr(), world)
            d.sync()
        ora.step_world(world)
        for d in devs:
            assert_same_state(d, ora, f"step {s}", counters=False)
        # a rank counts the nodes and infosets of its own trees
        assert tuple(sum(c) for c in zip(*[d.counters() for d in devs])) == ora.counters()
    assert devs[0].epoch == 3


@pytest.mark.parametrize("sampling", ["external", "pluribus"])
def test_reference_seed_mode_with_caller_built_streams(gpu, sampling):
    # rp_mccfr_set_rng(RP_RNG_REFERENCE) with streams the caller wrote (the infoset id as 4 little-endian bytes); the 16-way chance
    # node in the middle of the tree carries a chance_info and is drawn by random_range(0..16) from its own stream
    g = GT.game("chance16_mid")
    dev, ora = pair(g, "linear", "linear", sampling, 333, seed=42)
    streams = g.hash_streams()
    assert streams.n_chance > 0
    dev.set_rng("reference", streams)
    ora.set_rng("reference", streams)
    run(dev, ora, "ordered", 3, "reference-seed")
    # the mode is live: the counter RNG draws other trees from the same seed
    cnt = oracle.OracleSolver(g, "linear", "linear", sampling, batch=333, seed=42, hyper=pruning_hyper())
    for _ in range(3):
        cnt.step()
    assert not np.array_equal(cnt.export()["visits"], ora.export()["visits"])


def test_16_way_chance_draws_on_the_device_are_the_restated_ones_exactly(gpu):
    # no statistical margin: outcome k of the root chance is taken by exactly the trees whose restated draw (rp_node_hash with key
    # 0x80000000 | state, rp_pick_uniform: tests/mccfr_hand.py) is k — all 16 outcomes, the last one included
    g = GT.game("chance16_root")
    seed, batch = 3, 4000
    want = [0] * 16
    for tree in range(batch):
        want[chance_draw(seed, 0, tree, 0, 16)] += 1
    assert min(want) > 0 and sum(want) == batch
    infos = [g.info_of((0, 1, ((0, k),), ())) for k in range(16)]
    dev = Solver(g, "linear", "linear", "external", batch=batch, seed=seed)
    assert dev.kernel_variant() == "lds"
    dev.step()
    rows = dev.export().reshape(g.n_infos, g.max_actions)
    assert [int(rows["visits"][i, 0]) for i in infos] == want
    assert [int(rows["visits"][i, 1]) for i in infos] == want

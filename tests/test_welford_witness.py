"""The host witness of the Welford replays (tests/welford_witness.py, ora_welford_witness) on chains whose answer is known, and the
oracle profile's set_rows.  CPU only: tests/test_gpu_resumed_update.py relies on these answers to prove that its inputs reach the
replays of csrc/mccfr_update.hpp and csrc/sparse.hip (k_apply_hot)."""
import numpy as np
import pytest

import oracle
import welford_witness as ww
from robopoker_amd import Game

N = 50_000
VISITS = [0, (1 << 24) - 1000, 1 << 31]


def ordinary(kind, n=N, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return (rng.standard_normal(n) * 100.0).astype(np.float32)
    if kind == "unit":
        return rng.choice(np.array([-1.0, 1.0], dtype=np.float32), n)
    return (0.25 * rng.integers(-8, 9, n)).astype(np.float32)  # the caller-built tables' terminal payoffs (tests/game_tables.py)


def test_tile_sizes_are_read_from_the_kernels():
    assert ww.table_tile() == 1024 and ww.hot_tile() == 64 and ww.hot_touches() == 128


@pytest.mark.parametrize("visits", VISITS)
@pytest.mark.parametrize("kind", ["normal", "unit", "quarters"])
@pytest.mark.parametrize("tile", [1024, 64])
def test_ordinary_chains_never_reach_a_replay(kind, visits, tile):
    c = ww.chain(ordinary(kind), 0.0, visits, tile)
    assert c.tiles == (N + tile - 1) // tile and c.n == N
    assert (c.unproven, c.notok) == (0, 0)
    assert not c.flags.any()


@pytest.mark.parametrize("visits", [0, (1 << 24) - 1000])
def test_payoffs_of_2_to_minus_100_are_unproven_in_every_tile(visits):
    p = ordinary("normal", 5000, seed=1) * np.float32(2.0 ** -100)
    assert np.isfinite(p).all() and np.count_nonzero(p) == p.size
    c = ww.chain(p, 0.0, visits, 1024)
    assert c.tiles == 5 and c.unproven == 5 and c.notok == 5
    assert (c.flags == ww.UNPROVEN | ww.NOTOK).all()


def test_payoffs_of_2_to_minus_70_break_the_precondition_but_not_the_proof():
    p = ordinary("normal", 5000, seed=2) * np.float32(2.0 ** -70)
    for tile in (1024, 64):
        c = ww.chain(p, 0.0, 0, tile)
        assert c.tiles == (5000 + tile - 1) // tile
        assert c.unproven == 0 and c.notok == c.tiles
    # the figure the case was chosen by: payoffs of size 1e-20 (below 2^-60 = 8.7e-19, quotients far above 2^-97)
    c = ww.chain(ordinary("unit", 5000, seed=3) * np.float32(1e-20), 0.0, 0, 1)
    assert (c.unproven, c.notok, c.tiles) == (0, 5000, 5000)


def test_tiles_whose_replay_matters():
    # 3 * 2^-149 over 6 is a tie between 0 and 2^-149: IEEE rounds to even (0), the second correction of rp_div_by_recip lands on
    # 2^-149.  Off the precondition (and unproven), as it must be
    p = np.array([3], dtype=np.uint32).view(np.float32)
    c = ww.chain(p, 0.0, 5, 64)
    assert (c.tiles, c.unproven, c.notok, c.off2) == (1, 1, 1, 1) and c.ev == 0.0
    assert int(c.flags[0]) | ww.OFF1 == ww.UNPROVEN | ww.NOTOK | ww.OFF1 | ww.OFF2
    # subnormal payoffs over small divisors: some quotients differ, each of them in a tile that is replayed
    rng = np.random.default_rng(8)
    c = ww.chain((rng.standard_normal(20000) * 100.0).astype(np.float32) * np.float32(2.0 ** -135), 0.0, 0, 1)
    off1, off2 = (c.flags & ww.OFF1) != 0, (c.flags & ww.OFF2) != 0
    assert c.off1 > 0 and c.off2 > 0
    assert not (off1 & ((c.flags & ww.UNPROVEN) == 0)).any() and not (off2 & ((c.flags & ww.NOTOK) == 0)).any()
    # ordinary payoffs: never
    for visits in VISITS:
        c = ww.chain(ordinary("normal"), 0.0, visits, 1)
        assert (c.off1, c.off2) == (0, 0)


def test_the_witness_walks_the_chain_with_plain_division():
    p = ordinary("normal", 3000, seed=4)
    ev, v = np.float32(0.75), (1 << 24) - 1500
    c = ww.chain(p, ev, v, 1024)
    for i, x in enumerate(p):
        ev = np.float32(ev + np.float32(np.float32(x - ev) / np.float32(np.uint32(v + i + 1))))
    assert c.ev.view(np.uint32) == ev.view(np.uint32)
    # an empty chain: no tiles, ev untouched
    e = ww.chain(np.zeros(0, np.float32), 0.75, 5, 64)
    assert (e.tiles, e.unproven, e.notok, float(e.ev)) == (0, 0, 0, 0.75)


@pytest.mark.parametrize("visits", VISITS)
def test_the_planted_chain_fails_in_exactly_one_middle_tile(visits):
    tile = ww.hot_tile()
    n = 5 * tile + 17
    c = ww.chain(ww.planted_payoffs(n, tile, 2, seed=5), 0.0, visits, tile)
    assert c.tiles == 6 and c.notok == 1
    assert c.flags[2] & ww.NOTOK and not (c.flags[[0, 1, 3, 4, 5]] & ww.NOTOK).any()


def test_table_chains_group_a_batch_by_infoset_in_application_order():
    g = Game("kuhn")
    ora = oracle.OracleSolver(g, "linear", "linear", "external", batch=8192, seed=3)
    before = ora.export()
    dec = ww.decisions_of(ora)
    listed = ora.batch()
    assert len(listed) == dec.size and [d["info"] for d in listed[:50]] == dec["info"][:50].tolist()
    assert np.array_equal(np.array([d["payoff"] for d in listed], np.float32).view(np.uint32), dec["payoff"].view(np.uint32))
    chains = ww.table_chains(dec, before, g.max_actions)
    assert chains.keys() == ww.table_chains(listed, before, g.max_actions).keys()
    assert sum(c.n for c in chains.values()) == dec.size
    assert all(g.player(i) == 0 for i in chains)  # epoch 0: walker 0's infosets only
    # each walker infoset is reached by a third of the trees: more than two full tiles and a partial one
    assert max(c.n for c in chains.values()) > 2 * ww.PTILE and all(c.n % ww.PTILE for c in chains.values())
    assert all((c.unproven, c.notok) == (0, 0) and c.tiles == -(-c.n // ww.PTILE) for c in chains.values())
    # the chain of the witness is the oracle's own: its final ev is the payoff the step leaves in the cell
    ora.step()
    after = ora.export().reshape(-1, g.max_actions)
    for i, c in chains.items():
        assert after["visits"][i, 0] == c.n and after["payoff"][i, 0].view(np.uint32) == c.ev.view(np.uint32)


def test_sparse_chains_follow_the_rows_of_a_batch():
    from robopoker_amd.sparse import synthetic_batch  # host-side generator (numpy)

    batch = synthetic_batch(6000, 40, 9, seed=11)
    chains = ww.sparse_chains(batch)
    counts = np.bincount(batch[0], minlength=40)
    assert {r: c.n for r, c in chains.items()} == {r: int(k) for r, k in enumerate(counts) if k}
    o = oracle.OracleProfile(40, 9, "linear", "linear")
    o.apply(batch)
    got = o.rows(np.arange(40))
    for r, c in chains.items():
        assert got["payoff"][r, 0].view(np.uint32) == c.ev.view(np.uint32) and (c.unproven, c.notok) == (0, 0)


def test_oracle_profile_set_rows_round_trips():
    A, n_rows = 9, 40
    o = oracle.OracleProfile(n_rows, A, "linear", "linear")
    rng = np.random.default_rng(6)
    rows = np.array([3, 0, 39, 17], dtype=np.uint32)
    enc = np.zeros((rows.size, A), dtype=oracle.ENC_DTYPE)
    for f in ("weight", "regret", "payoff"):
        enc[f] = rng.standard_normal((rows.size, A)).astype(np.float32)
    enc["visits"] = rng.integers(0, 1 << 32, (rows.size, A), dtype=np.uint64).astype(np.uint32)
    enc["visits"][0, 0], enc["payoff"][0, 1] = 0xFFFFFFFF, np.float32(2.0 ** -140)  # the top count and a subnormal keep their bits
    o.set_rows(rows, enc)
    got = o.rows(rows)
    for f in ("weight", "regret", "payoff", "visits"):
        assert np.array_equal(got[f].view(np.uint32), enc[f].view(np.uint32)), f
    untouched = o.rows([1])
    assert not untouched["visits"].any() and not untouched["weight"].any() and not untouched["payoff"].any()
    # a hydrated row is what the next batch starts from
    o.set_epoch((1 << 32) + 3)
    assert o.epoch() == (1 << 32) + 3

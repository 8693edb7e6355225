"""The MCCFR and sparse-profile updates on a RESUMED table, bit for bit against the oracle after every step.

Every other parity test starts from an empty table at epoch 0 and feeds payoffs of ordinary size, which never enters
  - the Welford replays: csrc/mccfr_update.hpp re-derives every quotient of a 1024-payoff tile (rp_div_by_recip1) and replays the
    tile with IEEE divisions when one is unproven; k_apply_hot (csrc/sparse.hip) does the same per 64-touch staging tile on the
    precondition rp_div_by_recip_ok.  Ordinary payoffs never fail either; payoffs of size 2^-100 / 2^-70 do, and are legal;
  - the plain path of an infoset / row whose cells differ in `visits` or in the bits of `payoff` (only a hand-made import does);
  - counts next to 2^24 (consecutive divisors round to the same float), at and above 2^31 (a signed conversion would go wrong) and
    next to 2^32, epochs above 2^24 and above 2^32 ((float)epoch, the discounts, the 64-bit epoch of the node hash), and pruned
    sampling after the default warm-up of 16 384 epochs.
Flagship::hydrate -> rp_mccfr_import / rp_profile_set_rows / set_epoch is how a blueprint with millions of visits per cell resumes.

No case can pass vacuously: each asserts through the host witness (tests/welford_witness.py: the oracle's own walk of a cell's chain
with plain division and rp_math.h's two criteria, no kernel code) that its input reaches the replays its name says — every tile, one
tile, or none — and that its counts stand where its name says.
"""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest
import torch

import game_tables as GT
import oracle
import welford_witness as ww
from robopoker_amd import Game, _lib
from robopoker_amd.mccfr import Solver
from robopoker_amd.sparse import DeviceBatch, SparseProfile, synthetic_batch

pytestmark = pytest.mark.gpu
FIELDS = ("visits", "regret", "weight", "payoff")
GAMES = ["kuhn", "leduc", "chance16_mid"]  # two compile-time skeletons and one game of the generic kernels
BATCH = 8192  # a walker infoset behind a three-way deal is reached by a third of the trees: two full 1024-payoff tiles and a partial one
TINY = 2.0 ** -100  # quotients below 2^-97: no proof
DEEP = 2.0 ** -120  # quotients that are subnormal: the corrections of the reciprocal path round twice, only the replay is right
SCHEDULES = [("linear", "linear"), ("discounted", "quadratic"), ("floored", "exponential")]
SPLIT, FUSED = {"RP_FOLD_SPLIT": "1"}, {"RP_FOLD_SPLIT": "0"}


def resumed_states(touches):
    """(visits of every cell, epoch, why).  touches: the most a cell can collect in the run, so that visits never wrap"""
    return [((1 << 24) - 1500, (1 << 24) - 2, "both counts cross 2^24 during the run"),
            ((1 << 31) - 1500, (1 << 32) + 3, "visits cross 2^31, a 64-bit epoch"),
            ((1 << 32) - 1 - touches, (1 << 32) + 3, "visits next to the top of u32 without wrapping")]


STATE_IDS = ["v2p24", "v2p31", "vtop", "vsmall"]
# not a resumed blueprint: where two cells of an infoset or row differ by one visit, the divisors differ in the third digit and a chain that
# took the wrong one shows in most cells (next to 2^24 such divisors mostly round to the same quotient)
SMALL = (1000, 5, "small counts, a divisor off by one is another quotient")


def same(a, b, what=""):
    for f in FIELDS:
        if a[f].dtype.kind == "f":  # equal bits would also be equal NaNs: a table never holds one
            assert not np.isnan(a[f]).any(), f"{what}: NaN in {f}"
        diff = np.count_nonzero(a[f].view(np.uint32) != b[f].view(np.uint32))
        assert diff == 0, f"{what}: {f} differs bitwise in {diff} cells"


def same_state(dev, ora, what):
    same(dev.export(), ora.export(), what)
    assert dev.epoch == ora.epoch, what


# ---- games --------------------------------------------------------------------------------------------------------------------------
class PayoffGame:
    """a built-in game or a FRESHLY built catalogue game (never game_tables' cached one) whose table carries terminal payoffs scaled
    per player before any solver sees it (both solvers copy the table at creation)"""

    def __init__(self, name, scale):
        if name in GT._SPECS:
            why, players, plan, dr, variant = GT._SPECS[name]
            self.base = GT.TableGame(players, plan, default_regret=dr, seed=zlib.crc32(name.encode()))  # as game_tables.game() does
        else:
            self.base = Game(name)
        t = self.base.table
        n = t.n_terminals * t.n_players
        pay = np.array(t.payoffs[:n], dtype=np.float32).reshape(-1, t.n_players) * np.asarray(scale, dtype=np.float32)
        assert np.isfinite(pay).all() and np.count_nonzero(pay) == np.count_nonzero(np.array(t.payoffs[:n]))  # nothing underflows
        self._payoffs = (C.c_float * n)(*pay.ravel().tolist())
        self.table = _lib.GameTable.from_buffer_copy(t)
        self.table.payoffs = self._payoffs
        self.n_infos, self.max_actions = t.n_infos, t.max_actions

    def n_actions(self, info):
        return self.base.n_actions(info)

    def player(self, info):
        return self.base.player(info)


def plain_game(name):
    return GT.game(name) if name in GT._SPECS else Game(name)


# ---- one checked step ---------------------------------------------------------------------------------------------------------------
def checked_step(dev, ora, g, what, composed=False):
    """the witness of the step's batch against the table BEFORE it, then the step on both sides and the tables bit for bit"""
    before = ora.export()
    chains = ww.table_chains(ww.decisions_of(ora), before, g.max_actions)
    walker = ora.epoch % g.table.n_players
    assert chains and all(g.player(i) == walker for i in chains), what
    dev.step()
    if composed:
        ora.step_world(1)
    else:
        ora.step()
    same_state(dev, ora, what)
    return walker, chains, before.reshape(-1, g.max_actions)


def long_partial(chains):
    """a chain of more than two full tiles whose last tile is partial"""
    return any(c.n > 2 * ww.PTILE and c.n % ww.PTILE for c in chains.values())


def pair(g, regret, weight, sampling="external", batch=BATCH, seed=41, mode="ordered", hyper=None):
    dev = Solver(g, regret, weight, sampling, batch=batch, seed=seed, hyper=hyper)
    ora = oracle.OracleSolver(g, regret, weight, sampling, batch=batch, seed=seed, hyper=hyper)
    if mode == "composed":
        dev.set_update_mode("composed")
    return dev, ora


# ---- a. table games, ordered update: tiny payoffs -----------------------------------------------------------------------------------
@pytest.mark.parametrize("regret,weight,scale", [("linear", "linear", TINY), ("discounted", "quadratic", TINY), ("linear", "linear", DEEP)],
                         ids=["linear-linear-2p-100", "discounted-quadratic-2p-100", "linear-linear-2p-120"])
@pytest.mark.parametrize("name", GAMES)
def test_tiny_payoffs_replay_every_welford_tile(gpu, name, regret, weight, scale):
    assert ww.table_tile() == ww.PTILE
    g = PayoffGame(name, [scale, scale])
    dev, ora = pair(g, regret, weight)
    seen_long, mattered = False, 0
    for s in range(4):  # both walkers act twice: the second time from the ev the replays left
        walker, chains, _ = checked_step(dev, ora, g, f"{name} x {scale}, step {s}")
        # the input does what the name says: every tile of every chain holds an unproven quotient, so every tile is replayed
        assert all(c.tiles > 0 and c.unproven == c.tiles for c in chains.values()), (s, chains)
        seen_long |= long_partial(chains)
        mattered += sum(c.off1 for c in chains.values())
    assert seen_long
    if scale == DEEP:  # tiles in which the reciprocal path's own quotient is NOT the IEEE one: without the replay the table differs
        assert mattered > 0
    ex = ora.export()
    assert np.isfinite(ex["payoff"]).all() and np.count_nonzero(ex["payoff"]) > 0 and np.abs(ex["payoff"]).max() < 2.0 ** -90
    dev.close()


@pytest.mark.parametrize("name", GAMES)
def test_one_players_tiny_payoffs_replay_and_hand_back(gpu, name):
    # only player 0's payoffs are tiny: walker 0's steps replay every tile, walker 1's steps stay on the reciprocal path
    g = PayoffGame(name, [TINY, 1.0])
    dev, ora = pair(g, "linear", "linear")
    replayed, fast, seen_long = [0, 0], [0, 0], False
    for s in range(4):
        walker, chains, _ = checked_step(dev, ora, g, f"{name}, player 0 x 2^-100, step {s}")
        replayed[walker] += sum(c.unproven for c in chains.values())
        fast[walker] += sum(c.tiles - c.unproven for c in chains.values())
        seen_long |= long_partial(chains)
    assert replayed[0] > 0 and fast[0] == 0, (replayed, fast)
    assert replayed[1] == 0 and fast[1] > 0, (replayed, fast)
    assert seen_long
    dev.close()


# ---- a. table games, ordered update: hydrated ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def resumed_rows(name):
    """the table of a 3-step oracle run (read-only): what the hydrated states are made from"""
    ora = oracle.OracleSolver(plain_game(name), "linear", "linear", "external", batch=BATCH, seed=17)
    for _ in range(3):
        ora.step()
    rows = ora.export()
    assert np.count_nonzero(rows["visits"]) > 0
    rows.setflags(write=False)
    return rows


def hydrated(g, rows, visits):
    """the rows with `visits` in every cell of every infoset (the padding past an infoset's actions stays empty)"""
    out = rows.copy().reshape(g.n_infos, g.max_actions)
    for i in range(g.n_infos):
        out["visits"][i, : g.n_actions(i)] = visits
    return out.reshape(-1)


def run_hydrated(dev, ora, g, rows, epoch, steps, what, composed=False):
    dev.load_rows(rows, epoch)
    ora.load_rows(rows, epoch)
    same_state(dev, ora, f"{what}, hydrated")
    assert dev.epoch == epoch
    seen_long, failing_long, failing = False, 0, 0
    for s in range(steps):
        walker, chains, before = checked_step(dev, ora, g, f"{what}, step {s}", composed)
        assert walker == (epoch + s) % g.table.n_players
        seen_long |= long_partial(chains)
        failing_long += sum(c.unproven for c in chains.values() if c.n > 2 * ww.PTILE)
        failing += sum(c.unproven for c in chains.values())
    assert seen_long, what
    print(f"{what}: {failing} unproven tiles, {failing_long} of them in chains of more than two tiles")
    return failing_long


def assert_counts_stand_where_the_name_says(state, visits, epoch, ora, steps):
    after = ora.export()["visits"]
    top = int(after.max())
    assert top > visits and ora.epoch == epoch + steps  # no wrap: every count only grew
    if state == 0:
        assert visits < (1 << 24) < top and epoch < (1 << 24) < ora.epoch
        assert np.float32(visits + 1500) == np.float32(visits + 1501)  # consecutive divisors that round to the same float
    elif state == 1:
        assert visits < (1 << 31) < top and epoch > (1 << 32)
    else:
        assert (1 << 32) - (1 << 16) < visits < top <= (1 << 32) - 1 and epoch > (1 << 32)


@pytest.mark.parametrize("state", [0, 1, 2], ids=STATE_IDS[:3])
@pytest.mark.parametrize("regret,weight", SCHEDULES)
@pytest.mark.parametrize("name", GAMES)
def test_hydrated_tables_step_bit_exact(gpu, name, regret, weight, state):
    g = plain_game(name)
    visits, epoch, why = resumed_states(3 * BATCH)[state]
    dev, ora = pair(g, regret, weight)
    failing = run_hydrated(dev, ora, g, hydrated(g, resumed_rows(name), visits), epoch, 3, f"{name} {regret}/{weight}, {why}")
    # ordinary payoffs: the long chains stay on the reciprocal path at these divisors too (an infoset that is all but never reached
    # collects payoffs of size 1e-40, whose quotients are unproven in any table: a short chain)
    assert failing == 0
    assert_counts_stand_where_the_name_says(state, visits, epoch, ora, 3)
    dev.close()


def test_pluribus_prunes_after_the_default_warmup(gpu):
    # the default rp_hyper: prune_warmup 16 384 epochs, prune_threshold -3e5.  A hydrated epoch is past the warm-up, and the second
    # action of every infoset is hydrated at regret -4e5: pruned wherever its child is no terminal
    g = Game("leduc")
    hp = oracle.default_hyper()
    assert hp.prune_warmup == 16384 and hp.prune_threshold > -4e5 > hp.regret_min
    visits, epoch, why = resumed_states(3 * BATCH)[1]
    rows = hydrated(g, resumed_rows("leduc"), visits).reshape(g.n_infos, g.max_actions)
    unpruned = rows.copy().reshape(-1)
    rows["regret"][:, 1] = -4e5
    rows = rows.reshape(-1)
    dev, ora = pair(g, "linear", "linear", "pluribus")
    twin = oracle.OracleSolver(g, "linear", "linear", "pluribus", batch=BATCH, seed=41)
    twin.load_rows(unpruned, epoch)
    dev.load_rows(rows, epoch)
    ora.load_rows(rows, epoch)
    for s in range(3):
        dec = ww.decisions_of(ora)
        full = (1 << dec["n_actions"].astype(np.uint32)) - 1
        assert np.count_nonzero(dec["expanded"] != full) > 0, f"step {s}: no Decision with a pruned edge"
        dev.step()
        ora.step()
        twin.step()
        same_state(dev, ora, f"pluribus after the warm-up, step {s}")
        assert dev.counters() == ora.counters()
        assert ora.counters()[0] < twin.counters()[0], f"step {s}: the oracle visited no fewer nodes than without the hydrated regrets"
    dev.close()


# ---- a. table games, ordered update: non-uniform cells ------------------------------------------------------------------------------
def non_uniform(g, rows, popularity):
    """per infoset (by its rank in `popularity` modulo 3, so that the long chains are of all kinds): one action's visits raised by
    1 / one action's payoff moved by one ulp / untouched"""
    out = rows.copy().reshape(g.n_infos, g.max_actions)
    kind = np.zeros(g.n_infos, dtype=np.int64)
    kind[np.argsort(-popularity.astype(np.int64), kind="stable")] = np.arange(g.n_infos) % 3
    for i in range(g.n_infos):
        a = (i // 3) % g.n_actions(i)
        if kind[i] == 0:
            out["visits"][i, a] += 1
        elif kind[i] == 1:
            out["payoff"][i, a] = np.nextafter(out["payoff"][i, a], np.float32(np.inf))
    return out.reshape(-1), kind


@pytest.mark.parametrize("state", [0, 1, 3], ids=[STATE_IDS[i] for i in (0, 1, 3)])
def test_non_uniform_infosets_take_the_plain_path(gpu, state):
    name = "three_players_a5"  # 1, 2, 3 and 5 actions
    g = plain_game(name)
    assert g.max_actions >= 3
    visits, epoch, why = (resumed_states(3 * BATCH) + [SMALL])[state]
    popularity = resumed_rows(name).reshape(g.n_infos, g.max_actions)["visits"][:, 0]
    rows, kind = non_uniform(g, hydrated(g, resumed_rows(name), visits), popularity)
    dev, ora = pair(g, "linear", "linear")
    dev.load_rows(rows, epoch)
    ora.load_rows(rows, epoch)
    players = g.table.n_players
    longest = [0, 0, 0]  # the longest chain met, by kind
    for s in range(players + 1):  # every walker once from the planted cells, the first one again from what the plain path left
        walker, chains, before = checked_step(dev, ora, g, f"{name} non-uniform, {why}, step {s}")
        if s < players:  # the input does what the name says: the cells of the touched infosets differ as planted
            many = np.array([i for i in sorted(chains) if g.n_actions(i) > 1])
            differ_v = np.array([len(set(before["visits"][i, : g.n_actions(i)].tolist())) > 1 for i in many])
            differ_p = np.array([len(set(before["payoff"][i, : g.n_actions(i)].view(np.uint32).tolist())) > 1 for i in many])
            assert np.array_equal(differ_v, kind[many] == 0) and np.array_equal(differ_p, kind[many] == 1)
            for i in many:
                longest[kind[i]] = max(longest[kind[i]], chains[i].n)
    # all three kinds were stepped, the two plain ones with a chain of more than a tile
    assert longest[0] > ww.PTILE and longest[1] > ww.PTILE and longest[2] > 0, longest
    dev.close()


# ---- b. sparse profile, ordered -----------------------------------------------------------------------------------------------------
N_ROWS, A, TOUCHES = 40, 9, 6000
PAIRS = [("linear", "linear"), ("floored", "linear"), ("summed", "constant"), ("discounted", "quadratic"), ("asymmetric", "exponential")]
ALL_ROWS = np.arange(N_ROWS)


def hot_rows(batch):
    """rows that go to k_apply_hot, with their touch counts; asserts the batch has hot rows of more than two staging tiles (one of
    them partial) next to rows that stay in k_apply"""
    HT, HOT = ww.hot_tile(), ww.hot_touches()
    counts = np.bincount(batch[0], minlength=N_ROWS)
    hot = np.flatnonzero(counts > HOT)
    assert len(batch[0]) == TOUCHES and counts.max() > 2 * HT and hot.size >= 6
    assert np.count_nonzero((counts > 0) & (counts <= HOT)) >= 6
    assert any(counts[r] > 2 * HT and counts[r] % HT for r in hot)
    return hot, counts


def sparse_state(visits, seed, payoff=None):
    """hydrated rows: the same visits in every cell, regrets, weights and (unless stated) one payoff per row of ordinary size"""
    rng = np.random.default_rng(seed)
    enc = np.zeros((N_ROWS, A), dtype=oracle.ENC_DTYPE)
    enc["regret"] = (rng.standard_normal((N_ROWS, A)) * 500.0).astype(np.float32)
    enc["weight"] = (rng.random((N_ROWS, A)) * 1000.0 + 1.0).astype(np.float32)
    enc["payoff"] = (rng.standard_normal((N_ROWS, 1)) * 30.0).astype(np.float32) if payoff is None else np.float32(payoff)
    enc["visits"] = visits
    return enc


def sparse_pair(regret, weight, enc, epoch):
    g = SparseProfile(N_ROWS, A, regret, weight)
    o = oracle.OracleProfile(N_ROWS, A, regret, weight)
    g.set_rows(ALL_ROWS, enc)
    o.set_rows(ALL_ROWS, enc)
    g.set_epoch(epoch)
    o.set_epoch(epoch)
    same(g.rows(ALL_ROWS), o.rows(ALL_ROWS), "hydrated")
    return g, o


def rewritten(batch, counts, step, tiny):
    """the payoff column rewritten per row (by id modulo 3): all x tiny / planted (first batch only) / ordinary"""
    HT = ww.hot_tile()
    payoff = batch[5].copy()
    planted = []
    for r in range(N_ROWS):
        at = np.flatnonzero(batch[0] == r)  # the row's touches in application order
        if r % 3 == 0:
            payoff[at] *= np.float32(tiny)
        elif r % 3 == 1 and step == 0 and counts[r] > 2 * HT:
            tiles = -(-counts[r] // HT)
            payoff[at] = ww.planted_payoffs(counts[r], HT, tiles // 2, seed=r)
            planted.append(r)
    return batch[:5] + (payoff,), planted


# payoffs below the precondition; subnormal payoffs over small divisors, where rp_div_by_recip's quotient is not always the IEEE one
@pytest.mark.parametrize("tiny,visits", [(2.0 ** -70, 1000), (2.0 ** -135, 0)], ids=["2p-70", "2p-135"])
@pytest.mark.parametrize("regret,weight", PAIRS)
def test_hot_rows_replay_the_tiles_the_witness_names(gpu, regret, weight, tiny, visits):
    HT = ww.hot_tile()
    enc = sparse_state(visits, seed=3, payoff=0.0)  # payoff 0: the planted rows' zero payoffs leave zero numerators
    g, o = sparse_pair(regret, weight, enc, epoch=5)
    mattered = 0
    for step in range(2):  # the second batch starts from the ev the replays left
        raw = synthetic_batch(TOUCHES, N_ROWS, A, seed=70 + step)
        hot, counts = hot_rows(raw)
        batch, planted = rewritten(raw, counts, step, tiny)
        before = o.rows(ALL_ROWS)
        chains = ww.sparse_chains(batch, {r: before[r] for r in range(N_ROWS)})
        tiny_rows = [r for r in hot if r % 3 == 0]
        ordinary = [r for r in hot if r % 3 == 2]
        assert tiny_rows and ordinary
        assert all(chains[r].tiles > 2 and chains[r].notok == chains[r].tiles for r in tiny_rows)  # every staging tile is replayed
        assert all(chains[r].notok == 0 for r in ordinary)  # none is
        mattered += sum(chains[r].off2 for r in tiny_rows)
        if step == 0:
            assert planted and set(planted) <= set(hot.tolist())
            for r in planted:  # exactly one, neither the first nor the last: the tiles around it stay on the reciprocal path
                c = chains[r]
                assert c.notok == 1 and c.tiles >= 3 and not c.flags[0] & ww.NOTOK and not c.flags[-1] & ww.NOTOK, (r, c)
        g.apply(DeviceBatch(*batch), "ordered")
        o.apply(batch)
        g.sync()
        same(g.rows(ALL_ROWS), o.rows(ALL_ROWS), f"{regret}/{weight}, batch {step}")
    assert g.epoch() == o.epoch() == 7
    if visits == 0:  # tiles in which rp_div_by_recip's quotient is NOT the IEEE one: without the replay the table differs
        assert mattered > 0
    g.close()


def sparse_non_uniform(enc, nact):
    """per row (by id modulo 3): untouched / one action's visits raised by 1 (shared_v false) / one action's payoff moved by one ulp"""
    out = enc.copy()
    for r in range(N_ROWS):
        a = (r // 3) % int(nact[r])
        if r % 3 == 1:
            out["visits"][r, a] += 1
        elif r % 3 == 2:
            out["payoff"][r, a] = np.nextafter(out["payoff"][r, a], np.float32(np.inf))
    return out


def row_nact(batch):
    nact = np.full(N_ROWS, 2)
    nact[batch[0]] = batch[1]
    return nact


ORDERED_CASES = [(r, w, i % 3) for i, (r, w) in enumerate(PAIRS)] + [("linear", "linear", 3), ("discounted", "quadratic", 3)]


@pytest.mark.parametrize("regret,weight,state", ORDERED_CASES, ids=[f"{r}-{w}-{STATE_IDS[i]}" for r, w, i in ORDERED_CASES])
def test_hydrated_profile_applies_ordered_bit_exact(gpu, regret, weight, state):
    steps = 2
    visits, epoch, why = (resumed_states(steps * TOUCHES + 1) + [SMALL])[state]
    batches = [synthetic_batch(TOUCHES, N_ROWS, A, seed=90 + s) for s in range(steps)]
    enc = sparse_non_uniform(sparse_state(visits, seed=state), row_nact(batches[0]))
    g, o = sparse_pair(regret, weight, enc, epoch)
    for s, batch in enumerate(batches):
        hot, counts = hot_rows(batch)
        before = o.rows(ALL_ROWS)
        chains = ww.sparse_chains(batch, {r: before[r] for r in range(N_ROWS)})
        # hot rows of all three kinds; ordinary payoffs: no numerator of a uniform row leaves the precondition
        assert all(any(r % 3 == k for r in hot) for k in range(3))
        assert all(chains[r].notok == 0 for r in hot if r % 3 == 0)
        for r in hot:
            na = int(row_nact(batch)[r])
            assert (len(set(before["visits"][r, :na].tolist())) > 1) == (r % 3 == 1), r
            if s == 0:
                assert (len(set(before["payoff"][r, :na].view(np.uint32).tolist())) > 1) == (r % 3 == 2), r
        g.apply(DeviceBatch(*batch), "ordered")
        o.apply(batch)
        g.sync()
        same(g.rows(ALL_ROWS), o.rows(ALL_ROWS), f"{regret}/{weight}, {why}, batch {s}")
    after = o.rows(ALL_ROWS)["visits"]
    assert int(after.max()) > visits and int(after.min()) >= visits and g.epoch() == o.epoch() == epoch + steps
    if state == 0:
        assert visits < (1 << 24) < int(after.max()) and epoch < (1 << 24) <= o.epoch()
    elif state == 1:
        assert visits < (1 << 31) < int(after.max())
    g.close()


# ---- c. composed ----------------------------------------------------------------------------------------------------------------------
COMPOSED_BATCH = 16385  # 64 blocks of 256 trees, and a second group of one tree
COMPOSED_SCHEDULES = [("linear", "linear"), ("floored", "exponential"), ("summed", "quadratic")]


def composed_pair(monkeypatch, env, g, regret, weight, batch=COMPOSED_BATCH):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dev = Solver(g, regret, weight, "external", batch=batch, seed=43)
    for k in env:
        monkeypatch.delenv(k)
    dev.set_update_mode("composed")
    assert dev.fold_variant() == ("split" if env is SPLIT else "fused")
    return dev, oracle.OracleSolver(g, regret, weight, "external", batch=batch, seed=43)


@pytest.mark.parametrize("state", [0, 1, 2], ids=STATE_IDS[:3])
@pytest.mark.parametrize("env", [FUSED, SPLIT], ids=["fused", "split"])
@pytest.mark.parametrize("name", ["kuhn", "leduc"])
def test_hydrated_tables_step_composed_bit_exact(gpu, monkeypatch, name, env, state):
    g = Game(name)
    regret, weight = COMPOSED_SCHEDULES[state]
    visits, epoch, why = resumed_states(3 * COMPOSED_BATCH)[state]
    dev, ora = composed_pair(monkeypatch, env, g, regret, weight)
    run_hydrated(dev, ora, g, hydrated(g, resumed_rows(name), visits), epoch, 3, f"{name} composed {regret}/{weight}, {why}", composed=True)
    after = int(ora.export()["visits"].max())
    assert after > visits and ora.epoch == epoch + 3
    if state == 0:
        assert visits < (1 << 24) < after and epoch < (1 << 24) < ora.epoch
    elif state == 1:
        assert visits < (1 << 31) < after
    dev.close()


@pytest.mark.parametrize("env", [FUSED, SPLIT], ids=["fused", "split"])
@pytest.mark.parametrize("name", ["kuhn", "leduc"])
def test_tiny_payoffs_step_composed_bit_exact(gpu, monkeypatch, name, env):
    g = PayoffGame(name, [TINY, TINY])
    dev, ora = composed_pair(monkeypatch, env, g, "linear", "linear")
    for s in range(4):
        walker, chains, _ = checked_step(dev, ora, g, f"{name} x 2^-100 composed, step {s}", composed=True)
        # the same input that replays the tiles of the ordered update (all but a few one-tile chains of one repeated payoff)
        assert all(c.unproven == c.tiles for c in chains.values() if c.n > ww.PTILE)
        assert sum(c.unproven for c in chains.values()) > 0.9 * sum(c.tiles for c in chains.values())
    ex = ora.export()
    assert np.isfinite(ex["payoff"]).all() and np.count_nonzero(ex["payoff"]) > 0 and np.abs(ex["payoff"]).max() < 2.0 ** -90
    dev.close()


def summarized(g, o, batch, what):
    """one rank's entries from the device, byte for byte the oracle's; returns the blob"""
    db = DeviceBatch(*batch)
    buf = torch.zeros(db.n * g.entry_bytes(), dtype=torch.uint8, device="cuda")
    n = g.summarize(db, buf.data_ptr())
    g.sync()
    want = o.summarize(batch)
    assert n * g.entry_bytes() == want.size, what
    assert np.array_equal(buf[: want.size].cpu().numpy(), want), f"{what}: summary entries differ"
    return want


@pytest.mark.parametrize("tiny", [False, True], ids=["ordinary", "tiny"])
@pytest.mark.parametrize("state", [0, 1, 2], ids=STATE_IDS[:3])
def test_hydrated_profile_composed_apply_summarize_and_fold(gpu, state, tiny):
    regret, weight = COMPOSED_SCHEDULES[state]
    visits, epoch, why = resumed_states(3 * TOUCHES + 1)[state]
    batches = [synthetic_batch(TOUCHES, N_ROWS, A, seed=120 + s) for s in range(3)]
    if tiny:
        batches = [b[:5] + (b[5] * np.float32(2.0 ** -70),) for b in batches]
        assert all(c.notok == c.tiles for c in ww.sparse_chains(batches[0]).values())
    enc = sparse_non_uniform(sparse_state(visits, seed=10 + state, payoff=0.0 if tiny else None), row_nact(batches[0]))
    g, o = sparse_pair(regret, weight, enc, epoch)
    assert g.entry_bytes() == o.entry_bytes()
    hot_rows(batches[0])
    what = f"composed {regret}/{weight}, {why}"
    # one rank: its entries, then the local composed apply
    blob = summarized(g, o, batches[0], what)
    g.apply(DeviceBatch(*batches[0]), "composed")
    o.fold(blob)
    g.sync()
    same(g.rows(ALL_ROWS), o.rows(ALL_ROWS), f"{what}, apply")
    # two ranks: both entry lists, folded in rank order
    blobs = np.concatenate([summarized(g, o, b, what) for b in batches[1:]])
    dev = torch.from_numpy(blobs).cuda()
    g.fold(dev.data_ptr(), blobs.size // g.entry_bytes())
    o.fold(blobs)
    g.sync()
    same(g.rows(ALL_ROWS), o.rows(ALL_ROWS), f"{what}, fold of two ranks")
    after = o.rows(ALL_ROWS)["visits"]
    assert int(after.max()) > visits and int(after.min()) >= visits and g.epoch() == o.epoch() == epoch + 2
    if state == 0:
        assert visits < (1 << 24) < int(after.max()) and epoch < (1 << 24) <= o.epoch()
    elif state == 1:
        assert visits < (1 << 31) < int(after.max())
    g.close()

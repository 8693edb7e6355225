"""Pins tests/nlhe_rollout_model.py, the model tests/test_gpu_nlhe_frontier.py compares the device against, without a GPU: the
corners whose answer is known without it, sample_biased against the analytic biased distribution, the counter streams, the 12-edge
freeze of the story, and the symbols and constants of the C ABI (rp_nlhe_frontier_payoffs and its _device form)."""
import ctypes as C
import itertools
import os
import re

import numpy as np

import nlhe_policy_model as PM
import nlhe_rollout_model as FM
import oracle_nlhe as ON
from robopoker_amd import _lib
from robopoker_amd.nlhe import FRONTIER_DTYPE, Frontier

F = np.float32
OPEN2, POT = ON.Open(2), ON.RaiseOdds(1, 1)
DRAW, FOLD, CHECK, CALL, SHOVE = ON.E_DRAW, ON.E_FOLD, ON.E_CHECK, ON.E_CALL, ON.E_SHOVE


def cards(*cs):
    return sum(1 << c for c in cs)


HOLES = (cards(51, 50), cards(12, 25))


class NoRows:
    def get(self, key):
        raise AssertionError("a frontier without a decision asked for an infoset")


def test_a_terminal_frontier_is_its_settlement_in_every_cell():
    # seat 0 (the dealer: small blind) opens to 4, seat 1 folds its big blind: seat 0 wins 2, no draw is consumed
    for internal, want in ((0, 2.0), (1, -2.0)):
        f = Frontier(HOLES, internal, edges=[OPEN2, FOLD])
        status, pay, won = FM.payoffs(f, NoRows(), 0, rollouts=3, seed=7)
        assert status == FM.OK and (pay == F(want)).all() and (won == int(want)).all()
    game = FM.frontier_game(Frontier(HOLES, 0, edges=[OPEN2, FOLD]))
    stream = FM.Stream(7, 0)
    assert FM.rollout(game, (), 0, 3, 1, NoRows(), 5.0, stream) == 2 and stream.c == 0


def test_an_all_in_runout_is_the_mean_showdown_over_the_boards_its_draws_deal():
    f = Frontier(HOLES, 0, edges=[SHOVE, CALL])
    rollouts, seed, first_id, index = 3, 11, 5, 2
    status, pay, won = FM.payoffs(f, NoRows(), index, rollouts=rollouts, seed=seed, first_id=first_id)
    assert status == FM.OK
    o = ON.lib()
    boards = set()
    for k, j, r in itertools.product(range(4), range(4), range(rollouts)):
        # independently of the model's rollout: five cards by the counter contract, dealt at once, settled by the oracle
        rid = ((first_id + index) * 16 + 4 * k + j) * rollouts + r
        deck = [c for c in range(52) if not (HOLES[0] | HOLES[1]) >> c & 1]
        dealt = [1 << deck.pop(FM.pick_uniform(FM.node_hash(seed, 0, rid, c), len(deck))) for c in range(5)]
        streets = [dealt[0] | dealt[1] | dealt[2], dealt[3], dealt[4]]
        g = FM.frontier_game(f)
        for d in streets:
            assert o.ora_nlhe_apply(C.byref(g), C.byref(ON.ActionStruct(ON.DRAW, 0, d))) == 0
        out = C.c_float()
        assert o.ora_nlhe_payoff(C.byref(g), 0, C.byref(out)) == 0
        assert won[4 * k + j, r] == int(out.value) and abs(out.value) in (0.0, 200.0)
        boards.add(g.board)
    assert len(boards) == 16 * rollouts  # every rollout its own stream
    for k, j in itertools.product(range(4), range(4)):
        total = F(0.0)
        for r in range(rollouts):
            total = F(total + F(won[4 * k + j, r]))
        assert pay[k, j] == F(total / F(rollouts))


def test_sample_biased_follows_the_analytic_biased_distribution():
    # a fixed policy over raise, shove, call, fold; N draws u = rp_u01 of the counter stream.  Slot a is hit with probability
    # q_a = p_a m_a / sum(p m) up to the 2^-24 grid of u and float32 rounding (both below 1e-6); its count is binomial(N, q_a)
    # with standard deviation sqrt(N q_a (1 - q_a)), and a count further than 5 of those from N q_a has probability below 6e-7 per
    # slot — 16 slots are tested.  N = 20 000: 5 sigma is at most 5 sqrt(N) / 2 = 354 counts, the grid contributes N 1e-6 < 1.
    n_draws, bias = 20_000, 5.0
    edges = [POT, SHOVE, CALL, FOLD]
    dist = np.array([0.1, 0.2, 0.3, 0.4], F)
    us = [FM.u01(FM.node_hash(3, 0, 99, c)) for c in range(n_draws)]
    for continuation in range(4):
        mult = np.array([float(FM.multiplier(continuation, e, bias)) for e in edges])
        assert list(mult) == [[1, 1, 1, 1], [1, 1, 1, 5], [1, 1, 5, 1], [5, 5, 1, 1]][continuation]
        q = dist.astype(np.float64) * mult
        q /= q.sum()
        counts = np.bincount([FM.sample_biased(dist, edges, continuation, bias, u) for u in us], minlength=4)
        sigma = np.sqrt(n_draws * q * (1 - q))
        assert (np.abs(counts - n_draws * q) <= 5 * sigma + 1).all(), (continuation, counts, n_draws * q)
    # the scan's corners: u = 0 takes the first slot with weight, no slot above the threshold takes the last
    assert FM.sample_biased(np.array([0.0, 1.0], F), [CALL, FOLD], 0, bias, F(0.0)) == 1
    assert FM.sample_biased(np.array([np.nan, np.nan], F), [CALL, FOLD], 0, bias, F(0.5)) == 1


def test_streams_of_different_cells_share_no_draw():
    rollouts, first_id = 3, 4
    ids = [FM.rollout_id(first_id, i, k, j, rollouts, r) for i in range(3) for k in range(4) for j in range(4) for r in range(rollouts)]
    assert ids == list(range(first_id * 16 * rollouts, (first_id + 3) * 16 * rollouts))  # dense and distinct
    draws = {FM.node_hash(9, 0, rid, c) for rid in ids for c in range(8)}
    assert len(draws) == len(ids) * 8
    # frontier i of a call with first_id f is frontier 0 of a call with first_id f + i; ids wrap
    assert FM.rollout_id(4, 2, 3, 1, 3, 2) == FM.rollout_id(6, 0, 3, 1, 3, 2)
    assert FM.rollout_id((1 << 64) - 1, 1, 0, 0, 3, 0) == 0


def test_the_story_freezes_after_twelve_edges_and_that_changes_the_key():
    # a river decision reached with an 11-edge story: the 12th edge (a check) still enters the key, the 13th (a pot bet) does not
    f = Frontier(HOLES, 0, [cards(3, 17, 30), cards(44), cards(9)],
                 [OPEN2, CALL, DRAW, CHECK, CHECK, DRAW, CHECK, CHECK, DRAW, CHECK, POT])
    g = FM.frontier_game(f)
    turn = ON.lib().ora_nlhe_turn(C.byref(g))
    assert turn in (0, 1)
    story = list(f.edges)
    assert len(story) == 11
    k11 = FM.key_at(g, story, turn)
    k12 = FM.key_at(g, story + [CHECK], turn)
    k13 = FM.key_at(g, story + [CHECK, POT], turn)
    assert ON.path_unpack(k11[0]) == [CHECK, POT] and ON.path_unpack(k12[0]) == [CHECK, POT, CHECK]
    assert k13 == k12  # frozen: the 13th edge is dropped ...
    unfrozen = ON.lib().ora_path_aggression(ON.path_pack([CHECK, POT, CHECK, POT]))
    assert unfrozen == 2 and ON.lib().ora_path_aggression(k13[0]) == 1  # ... although it would have changed past and aggression
    # and a rollout from an 11-edge prefix meets it: some decision is keyed with a story longer than 12
    used = []
    rows = {}
    for r in range(12):
        FM.rollout(g, tuple(f.edges), 0, 3, 3, rows, 5.0, FM.Stream(1, r), used)
    assert any(length > 12 for _, _, length in used)


def test_validation_statuses():
    ok = dict(holes=HOLES, internal=0, draws=[cards(3, 17, 30)], edges=[OPEN2, CALL, DRAW])
    cases = [
        (dict(ok, holes=(cards(51, 50), cards(50, 25))), FM.CARDS),
        (dict(ok, holes=(cards(51, 50), cards(3, 25))), FM.CARDS),
        (dict(ok, holes=(cards(51, 50, 49), cards(12, 25))), FM.CARDS),
        (dict(ok, edges=[OPEN2, CALL, DRAW, 25]), FM.EDGE),
        (dict(ok, prefix=[0]), FM.EDGE),
        (dict(ok, prefix=[CHECK] * 13), FM.LENGTH),
        (dict(ok, edges=[CHECK] * 49), FM.LENGTH),
        (dict(ok, internal=2), FM.SEAT),
        (dict(ok, stacks=(10, 0)), FM.SEAT),
        (dict(ok, draws=[]), FM.DRAW),
        (dict(ok), FM.OK),
    ]
    for kw, want in cases:
        status, pay, won = FM.payoffs(Frontier(**kw), {}, 0, rollouts=1)
        assert status == want, (kw, status)
        assert want == FM.OK or (not pay.any() and not won.any())


def test_abi_symbols_and_constants():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "rp_mi355x.h")).read()
    for name in ("rp_nlhe_frontier_payoffs", "rp_nlhe_frontier_payoffs_device"):
        assert re.search(r"RP_API int %s\(" % name, header) and name in _lib.declared_symbols()
        assert hasattr(_lib.load(), name)
    assert re.search(r"#define\s+RP_NLHE_FRONTIER_LEAVES\s+4u", header) and re.search(r"#define\s+RP_NLHE_MAX_PREFIX\s+12u", header)
    assert (_lib.RP_NLHE_FRONTIER_LEAVES, _lib.RP_NLHE_MAX_PREFIX) == (FM.LEAVES, FM.MAX_PREFIX) == (4, 12)
    assert FRONTIER_DTYPE.itemsize == C.sizeof(_lib.NlheFrontier) == 112
    for field in FRONTIER_DTYPE.names:  # the numpy record and the ctypes struct agree field by field
        assert FRONTIER_DTYPE.fields[field][1] == getattr(_lib.NlheFrontier, field).offset, field
    packed = Frontier.pack([Frontier(HOLES, 1, [7], [OPEN2, CALL, DRAW], [CHECK], (150, 90))])
    assert packed["n_edges"][0] == 3 and packed["n_prefix"][0] == 1 and packed["internal"][0] == 1 and list(packed["stacks"][0]) == [150, 90]
    # arguments are refused before any device work: a NULL handle, on a machine without a GPU too
    lib = _lib.load()
    assert lib.rp_nlhe_frontier_payoffs(None, 0, None, 5.0, 16, 0, 0, None, None, None) == _lib.RP_ERR_INVALID

"""Frontier payoffs from the device-resident blueprint: rp_nlhe_frontier_payoffs, host and _device forms, against the naive
one-game-per-rollout model of tests/nlhe_rollout_model.py (pinned by tests/test_nlhe_rollout_model.py).  Bit patterns only: there is no
tolerance.

One batch (rollouts = 3) mixes every kind of frontier: the preflop root, a chance frontier whose prefix is its history, a flop chance
frontier with uneven stacks and a prefix that is no suffix of its history, the other seat as `internal`, a river decision whose
11-edge prefix lets the path saturate inside the rollout, a fold, an all-in runout, a frontier none of whose infosets has a row, and
three malformed records between valid ones.  The table is built from the keys the model asks for: about half of them get a row
(chosen by a hash of the key), some of those all zero, in the smallest power of two of slots above twice the rows.  Found, absent,
off-home-slot, zero-row and saturated-path decisions are each asserted to occur."""
import ctypes as C

import numpy as np
import pytest
import torch

import nlhe_policy_model as PM
import nlhe_read_chunk as RC
import nlhe_rollout_model as FM
import oracle_nlhe as ON
from robopoker_amd import _lib
from robopoker_amd.nlhe import A, ENC_DTYPE, Frontier, NlheSolver

pytestmark = pytest.mark.gpu

WEIGHTS = np.array([0.0, 1e-39, 1.0, 1e12], np.float32)  # 1e-39 is subnormal: below RP_EPSILON
OPEN2, OPEN3, POT, HALF = ON.Open(2), ON.Open(3), ON.RaiseOdds(1, 1), ON.RaiseOdds(1, 2)
DRAW, FOLD, CHECK, CALL, SHOVE = ON.E_DRAW, ON.E_FOLD, ON.E_CHECK, ON.E_CALL, ON.E_SHOVE
BIAS, ROLLOUTS, SEED, FIRST_ID = 5.0, 3, 0x5EED, 1000
STRIDE_ROLLOUTS = 70  # 16 x 70 = 1 120 rollouts: more than the 256 lanes of a workgroup


def cards(*cs):
    return sum(1 << c for c in cs)


HOLES, FLOP, TURN, RIVER = (cards(51, 50), cards(12, 25)), cards(3, 17, 30), cards(44), cards(9)
TO_THE_RIVER = [OPEN2, CALL, DRAW, CHECK, CHECK, DRAW, CHECK, CHECK, DRAW, CHECK, POT]  # 11 edges, seat 1 to answer a river bet
# (name, frontier); the absent frontier comes first: its keys are never loaded, whoever else asks for them
CASES = [
    ("absent", Frontier((cards(0, 1), cards(20, 33)), 0, [cards(21, 22, 23)], [OPEN3, CALL, DRAW])),
    ("root", Frontier(HOLES, 0)),
    ("chance", Frontier(HOLES, 0, edges=[OPEN2, CALL], prefix=[OPEN2, CALL])),
    ("flop chance", Frontier(HOLES, 0, [FLOP], [OPEN2, CALL, DRAW, CHECK, HALF, CALL], [CHECK, POT], stacks=(150, 90))),
    ("overlapping holes", Frontier((cards(51, 50), cards(50, 25)), 0, edges=[OPEN2, CALL])),
    ("internal 1", Frontier(HOLES, 1, edges=[OPEN2, CALL], prefix=[OPEN2, CALL])),
    ("river", Frontier(HOLES, 0, [FLOP, TURN, RIVER], TO_THE_RIVER, TO_THE_RIVER)),
    ("bad edge", Frontier(HOLES, 0, [FLOP], [OPEN2, CALL, DRAW, 25])),
    ("fold", Frontier(HOLES, 0, edges=[OPEN2, FOLD])),
    ("all in", Frontier(HOLES, 1, edges=[SHOVE, CALL])),
    ("long prefix", Frontier(HOLES, 0, edges=[OPEN2, CALL], prefix=[CHECK] * 13)),
]
NAMES = [c[0] for c in CASES]
STATUS = {"overlapping holes": FM.CARDS, "bad edge": FM.EDGE, "long prefix": FM.LENGTH}
STRIDE = Frontier(HOLES, 0, [FLOP, TURN, RIVER], TO_THE_RIVER, [CHECK, POT])


class Rows:
    """the blueprint the model reads, decided key by key as the model asks: about half of the keys get a row of corner weights
    (garbage beyond the infoset's actions), the others — and every key the absent frontier asked for — have none"""

    def __init__(self):
        self.loaded, self.never, self.forbid = {}, set(), False

    def get(self, key):
        if self.forbid:
            self.never.add(key)
        if key in self.never:
            return None
        if key not in self.loaded:
            h = PM.key_hash(key[0] ^ 0x5EED, key[2], key[1])
            w = None
            if h % 2 == 0:
                w = WEIGHTS[[(h >> (8 + 2 * a)) & 3 for a in range(A)]].copy()
                if (h >> 40) % 8 == 0:
                    w[:] = 0.0  # a row whose weights are all zero: the same uniform policy as an absent one
                w[PM.nch(key[2]):] = 7.0
            self.loaded[key] = w
        return self.loaded[key]

    def table(self):
        keys = [k for k, w in self.loaded.items() if w is not None]
        enc = np.zeros((len(keys), A), dtype=ENC_DTYPE)
        enc["weight"] = np.stack([self.loaded[k] for k in keys])
        enc["regret"], enc["payoff"], enc["visits"] = -3.0, 2.5, 11
        return (np.array([k[0] for k in keys], np.uint64), np.array([k[1] for k in keys], np.uint32),
                np.array([k[2] for k in keys], np.uint64), enc)


class Model:
    """the model's answers for CASES and STRIDE, computed once per module"""

    def __init__(self):
        self.rows, self.used, self.want = Rows(), {}, []
        for i, (name, f) in enumerate(CASES):
            self.rows.forbid = name == "absent"
            self.used[i] = []
            self.want.append(FM.payoffs(f, self.rows, i, BIAS, ROLLOUTS, SEED, FIRST_ID, used=self.used[i]))
        self.rows.forbid = False
        self.stride = FM.payoffs(STRIDE, self.rows, 0, BIAS, STRIDE_ROLLOUTS, SEED, 7)
        self.table = self.rows.table()
        self.cap_log2 = (2 * self.table[0].size).bit_length()  # the power of two above twice the rows

    def solver(self):
        s = NlheSolver(cap_log2=self.cap_log2, batch=1, seed=1)
        s.load(*self.table, epoch=3)
        return s


@pytest.fixture(scope="module")
def model():
    return Model()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def frontiers():
    return [c[1] for c in CASES]


def on_device(fr):
    return torch.from_numpy(Frontier.pack(fr).view(np.uint8).copy()).to("cuda")


def equal(a, b):
    """two answers (payoffs, status, won) bit for bit"""
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def as_map(past, present, choices, enc):
    return {(int(p), int(q), int(c)): enc[i].tobytes() for i, (p, q, c) in enumerate(zip(past, present, choices))}


def test_every_case_occurs(model):
    m = model
    past, present, choices, enc = m.table
    slots = 1 << m.cap_log2
    assert 2 * past.size < slots <= 4 * past.size
    taken, off_home = set(), set()  # rp_nlhe_import into an empty table: insertion in order, linear probing
    for p, q, c in zip(past, present, choices):
        s = home = PM.key_hash(p, c, q) & (slots - 1)
        while s in taken:
            s = (s + 1) & (slots - 1)
        taken.add(s)
        if s != home:
            off_home.add((int(p), int(q), int(c)))
    everything = [u for i in m.used for u in m.used[i]]
    assert any(found and key in off_home for key, found, _ in everything), "no decision reads a row off its home slot"
    assert any(found for _, found, _ in everything) and any(not found for _, found, _ in everything)
    assert any(found and not m.rows.loaded[key][: PM.nch(key[2])].any() for key, found, _ in everything), "no all-zero row"
    assert any(found and (m.rows.loaded[key][: PM.nch(key[2])] == WEIGHTS[1]).any() for key, found, _ in everything), "no subnormal weight"
    absent = m.used[NAMES.index("absent")]
    assert absent and not any(found for _, found, _ in absent)
    river = m.used[NAMES.index("river")]
    assert any(length > FM.MAX_PREFIX for _, _, length in river), "no decision is keyed with a saturated path"
    assert not m.used[NAMES.index("fold")] and not m.used[NAMES.index("all in")]
    for i, name in enumerate(NAMES):
        status, pay, won = m.want[i]
        assert status == STATUS.get(name, FM.OK), name
        assert status == FM.OK or (not pay.any() and not won.any())
    fold = m.want[NAMES.index("fold")]
    assert (fold[1] == np.float32(2.0)).all() and (fold[2] == 2).all()
    assert set(np.unique(m.want[NAMES.index("all in")][2])) <= {-200, 0, 200}
    assert len(np.unique(m.want[NAMES.index("root")][2])) > 2  # the rollouts do end differently
    assert m.stride[0] == FM.OK and m.stride[2].shape == (16, STRIDE_ROLLOUTS)


def test_host_form_against_the_model(gpu, model):
    m = model
    s = m.solver()
    before = (as_map(*s.export()), s.epoch, s.counters())
    pay, status, won = s.frontier_payoffs(frontiers(), BIAS, ROLLOUTS, SEED, FIRST_ID, return_won=True)
    assert won.shape == (len(CASES), 16, ROLLOUTS) and won.dtype == np.int16
    for i, name in enumerate(NAMES):
        want_status, want_pay, want_won = m.want[i]
        assert status[i] == want_status, name
        assert np.array_equal(won[i], want_won), name
        assert np.array_equal(bits(pay[i]), bits(want_pay)), name
    # without the optional outputs
    only = s.frontier_payoffs(frontiers(), BIAS, ROLLOUTS, SEED, FIRST_ID)
    assert np.array_equal(bits(only[0]), bits(pay)) and np.array_equal(only[1], status)
    # read-only: the export as a map, the epoch and the counters; and the table still trains
    after = (as_map(*s.export()), s.epoch, s.counters())
    assert before == after and after[1:] == (3, (0, 0, m.table[0].size))
    s.step()
    assert s.epoch == 4 and s.counters()[2] >= m.table[0].size


def test_more_rollouts_than_lanes(gpu, model):
    m = model
    s = m.solver()
    pay, status, won = s.frontier_payoffs(STRIDE, BIAS, STRIDE_ROLLOUTS, SEED, 7, return_won=True)
    want_status, want_pay, want_won = m.stride
    assert status[0] == want_status == FM.OK
    assert np.array_equal(won[0], want_won) and np.array_equal(bits(pay[0]), bits(want_pay))


def test_device_form_splits_repeats_and_seeds(gpu, model):
    m = model
    s = m.solver()
    host = s.frontier_payoffs(frontiers(), BIAS, ROLLOUTS, SEED, FIRST_ID, return_won=True)
    dev = s.frontier_payoffs_device(on_device(frontiers()), BIAS, ROLLOUTS, SEED, FIRST_ID, return_won=True)
    s.sync()
    assert all(t.is_cuda for t in dev)
    assert equal([t.cpu().numpy() for t in dev], host)
    # the batch in two calls with matching first_id; the same call again
    cut = 4
    first = s.frontier_payoffs(frontiers()[:cut], BIAS, ROLLOUTS, SEED, FIRST_ID, return_won=True)
    second = s.frontier_payoffs(frontiers()[cut:], BIAS, ROLLOUTS, SEED, FIRST_ID + cut, return_won=True)
    assert equal([np.concatenate([a, b]) for a, b in zip(first, second)], host)
    assert equal(s.frontier_payoffs(frontiers(), BIAS, ROLLOUTS, SEED, FIRST_ID, return_won=True), host)
    # another seed plays other games (the fold and the malformed records answer as before)
    other = s.frontier_payoffs(frontiers(), BIAS, ROLLOUTS, SEED + 1, FIRST_ID, return_won=True)
    assert np.array_equal(other[1], host[1]) and not np.array_equal(other[2], host[2])
    assert np.array_equal(other[2][NAMES.index("fold")], host[2][NAMES.index("fold")])
    # rollouts = 0 is rollouts = 1
    assert equal(s.frontier_payoffs(frontiers(), BIAS, 0, SEED, FIRST_ID, return_won=True),
                 s.frontier_payoffs(frontiers(), BIAS, 1, SEED, FIRST_ID, return_won=True))


def test_arguments(gpu):
    lib = _lib.load()
    s = NlheSolver(cap_log2=10, batch=4, seed=2)
    fr = Frontier.pack([Frontier(HOLES, 0, edges=[OPEN2, FOLD])])
    pay, won, status = np.zeros((1, 4, 4), np.float32), np.zeros((1, 16, 16), np.int16), np.zeros(1, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for fn in (lib.rp_nlhe_frontier_payoffs, lib.rp_nlhe_frontier_payoffs_device):
        for bias in (0.0, -1.0, float("inf"), float("nan")):
            assert fn(s._h, 1, p(fr), bias, 16, 0, 0, p(pay), None, None) == _lib.RP_ERR_INVALID
        assert b"bias" in lib.rp_last_error()
        assert fn(s._h, 1, p(fr), 5.0, 4097, 0, 0, p(pay), None, None) == _lib.RP_ERR_INVALID
        assert b"rollouts" in lib.rp_last_error()
        assert fn(s._h, 0, None, 5.0, 16, 0, 0, None, None, None) == _lib.RP_OK
    assert lib.rp_nlhe_frontier_payoffs(s._h, 1, None, 5.0, 16, 0, 0, p(pay), None, None) == _lib.RP_ERR_INVALID
    assert lib.rp_nlhe_frontier_payoffs(s._h, 1, p(fr), 5.0, 16, 0, 0, None, None, None) == _lib.RP_ERR_INVALID
    # won and status may be NULL; an empty table answers a fold with its settlement
    assert lib.rp_nlhe_frontier_payoffs(s._h, 1, p(fr), 5.0, 16, 0, 0, p(pay), None, None) == _lib.RP_OK
    assert (pay == np.float32(2.0)).all()
    assert lib.rp_nlhe_frontier_payoffs(s._h, 1, p(fr), 5.0, 16, 0, 0, p(pay), p(won), p(status)) == _lib.RP_OK
    assert (won == 2).all() and status[0] == FM.OK
    # the largest number of rollouts a call takes, on a frontier that needs no lookup; the handle still steps
    pay4096, status4096 = s.frontier_payoffs(Frontier(HOLES, 1, edges=[OPEN2, FOLD]), rollouts=4096)
    assert (pay4096 == np.float32(-2.0)).all() and status4096[0] == FM.OK
    s.step()
    assert s.epoch == 1 and s.counters()[2] > 0


def test_the_payoffs_do_not_depend_on_the_launch_chunk(gpu, model):
    """RP_NLHE_READ_CHUNK (tests/nlhe_read_chunk.py) cuts the batch into launches of 1, 3, n - 1 and n frontiers: every launch counts its
    ids on from first_id and writes payoffs, won and status from its own item on"""
    m, s = model, model.solver()
    fr, n = frontiers(), len(CASES)
    dev_in = on_device(fr)
    call = lambda part, first_id: s.frontier_payoffs(part, BIAS, ROLLOUTS, SEED, first_id, return_won=True)
    with RC.read_chunk(None):
        want = call(fr, FIRST_ID)
    assert n % 16 and FIRST_ID and len(set(want[1])) == 4

    def against_the_model(got, what):
        for i, name in enumerate(NAMES):
            want_status, want_pay, want_won = m.want[i]
            assert got[1][i] == want_status and np.array_equal(got[2][i], want_won) and np.array_equal(bits(got[0][i]), bits(want_pay)), (what, name)

    for chunk in RC.cuts(n):
        with RC.read_chunk(chunk):
            host = call(fr, FIRST_ID)
            dev = s.frontier_payoffs_device(dev_in, BIAS, ROLLOUTS, SEED, FIRST_ID, return_won=True)
            s.sync()
        RC.same(host, want, (chunk, "host"))
        RC.same([t.cpu().numpy() for t in dev], want, (chunk, "device"))
        against_the_model(host, chunk)  # the river decision is the first frontier of the third launch of 3
        if chunk < n:  # the items from the first cut on: a call of their own under first_id + chunk, in one launch
            with RC.read_chunk(None):
                RC.same(call(fr[chunk:], FIRST_ID + chunk), RC.tail(want, chunk), (chunk, "ids"))
                assert chunk == n - 1 or not equal(call(fr[chunk:], FIRST_ID), RC.tail(want, chunk))  # the last frontier is malformed
    at = NAMES.index("river")
    with RC.read_chunk(1):  # one frontier: the status byte ends the staging arena off its alignment
        RC.same(call(fr[at: at + 1], FIRST_ID + at), [x[at: at + 1] for x in want], "one frontier")
    # won and status left out, in launches of 3
    lib, packed, pay = _lib.load(), Frontier.pack(fr), np.zeros((n, 4, 4), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    with RC.read_chunk(3):
        assert lib.rp_nlhe_frontier_payoffs(s._h, n, p(packed), BIAS, ROLLOUTS, SEED, FIRST_ID, p(pay), None, None) == _lib.RP_OK
    assert pay.tobytes() == want[0].tobytes()

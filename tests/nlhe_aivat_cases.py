"""The batch of hands the AIVAT tests share (helper, no tests), the blueprint it is evaluated against, and the model's answers with
their trace.  tests/test_nlhe_aivat_model.py asserts on the CPU that every case the kernel has to get right occurs in this batch;
tests/test_gpu_nlhe_aivat.py compares rp_nlhe_aivat with the model on it.

Heads-up, blinds 1 / 2: the dealer posts the small blind and acts first before the flop, the other seat acts first after it.  Chips
are what a play ADDS.  The blueprint is decided key by key as the model asks, by a hash of the key: about half of the infosets get
a row.  (With board_mode 0 a node before the hand's last street asks with the last street's bucket.  Where the betting so far and the
choices look the same on both streets that key IS the later street's infoset, and finds its row: the check that opens the turn and
the check that opens the river of the "streets" hands are one key.)"""
import numpy as np

import nlhe_aivat_model as AM
import nlhe_policy_model as PM
from robopoker_amd.nlhe import A, ENC_DTYPE, AivatHand

CAP_LOG2 = 10
SLOTS = 1 << CAP_LOG2
SALT = 2  # chosen so that every case of tests/test_nlhe_aivat_model.py::conditions occurs
WEIGHTS = np.array([0.0, 1e-39, 1.0, 1e12], np.float32)  # 1e-39 is subnormal
PAYOFFS = np.array([-1e20, -3.5, -1e-40, 0.25, 1e-40, 7.0, 1e20, -0.0], np.float32)  # both signs, large and subnormal; no sum overflows


def cards(*cs):
    return sum(1 << c for c in cs)


HOLES, FLOP, TURN, RIVER = (cards(12, 25), cards(38, 51)), cards(3, 17, 30), cards(44), cards(9)
BOARD = [FLOP, TURN, RIVER]
F_, X, C_, R, S = "fold", "check", "call", "raise", "shove"
# a bet and a call on every street down to a showdown; before the flop Raise(5) lies between Open(2) = 4 and Open(3) = 6 chips, on the
# river Raise(20) between 1/3 and 1/2 of the pot of 48: both snap to the FIRST of the two
STREETS = [(R, 5), (C_, 4), (X, 0), (R, 6), (C_, 6), (X, 0), (R, 12), (C_, 12), (X, 0), (R, 20), (C_, 20)]
# (name, hand); the absent hand comes first: its keys are never loaded, whoever else asks for them
CASES = [
    ("absent", AivatHand((cards(0, 1), cards(2, 4)), [cards(20, 21, 22), cards(40)], [(C_, 1), (X, 0), (X, 0), (X, 0), (X, 0), (X, 0)])),
    ("preflop fold", AivatHand(HOLES, (), [(F_, 0)])),
    ("streets seat 0", AivatHand(HOLES, BOARD, STREETS, seat=0)),
    ("witness refuses", AivatHand(HOLES, BOARD, [(S, 49), (C_, 48)], stacks=(50, 50))),
    ("streets seat 1", AivatHand(HOLES, BOARD, STREETS, seat=1)),
    # limped; on the flop (pot 4) Raise(7) is nearer to 2/1 = 8 than to 1/1 = 4 below it, and the fifth raise of the street meets an
    # empty grid (depth 4 > MAX_RAISE_REPEATS): Shove
    ("off grid", AivatHand(HOLES, BOARD, [(C_, 1), (X, 0), (R, 7), (R, 14), (R, 14), (R, 14), (R, 14), (C_, 7), (X, 0), (X, 0), (X, 0), (X, 0)], seat=1)),
    ("walker refuses", AivatHand(HOLES, BOARD, [(R, 30), (F_, 0)], stacks=(20, 20))),
    ("stacks", AivatHand(HOLES, BOARD[:2], [(R, 4), (C_, 3), (X, 0), (X, 0), (X, 0), (R, 5), (F_, 0)], seat=1, stacks=(150, 90), dealer=1)),
    ("bad kind", AivatHand(HOLES, BOARD, [(C_, 1), (9, 0)])),
    # the big blind's 198 are its whole stack: the rules know that call as a Shove
    ("all in", AivatHand(HOLES, BOARD, [(S, 199), (S, 198)])),
    # 16 edges with the Draws; the river re-raise is edge 15 of the history, snapped there with the aggression of its first 12 edges
    ("long", AivatHand(HOLES, BOARD, STREETS[:10] + [(R, 40), (C_, 20)], seat=1)),
    ("overlap", AivatHand((cards(12, 25), cards(3, 51)), BOARD, [(C_, 1), (X, 0), (X, 0), (X, 0)])),
    ("after a fold", AivatHand(HOLES, (), [(R, 4), (F_, 0), (X, 0), (C_, 2)], seat=1)),
    ("no flop", AivatHand(HOLES, (), [(C_, 1), (X, 0), (X, 0)])),
    ("streets at the node", AivatHand(HOLES, BOARD, STREETS, seat=0, board_mode=1)),
    ("both refuse", AivatHand(HOLES, BOARD, [(X, 0)])),
]
STATUS = {"witness refuses": AM.WITNESS, "walker refuses": AM.ILLEGAL, "bad kind": AM.EDGE, "overlap": AM.CARDS, "no flop": AM.DRAW,
          "both refuse": AM.ILLEGAL}
NAMES = [c[0] for c in CASES]


class Rows:
    """the blueprint the model reads"""

    def __init__(self, salt=SALT):
        self.loaded, self.never, self.forbid, self.n_rows, self.salt = {}, set(), False, 0, salt

    def get(self, key):
        if self.forbid:
            self.never.add(key)
        if key in self.never:
            return None
        if key not in self.loaded:
            h = PM.key_hash(key[0] ^ self.salt, key[2], key[1])
            row = None
            if h % 2 == 0 and self.n_rows < SLOTS - 64:
                self.n_rows += 1
                w = WEIGHTS[[(h >> (8 + 2 * a)) & 3 for a in range(A)]].copy()
                v = PAYOFFS[[(h >> (26 + 3 * a)) & 7 for a in range(A)]].copy()
                if (h >> 56) % 8 == 0:
                    w[:] = 0.0  # a row of zero total weight
                n = PM.nch(key[2])
                w[n:], v[n:] = 7.0, np.float32(np.inf)  # garbage past the infoset's actions
                row = (w, v)
            self.loaded[key] = row
        return self.loaded[key]

    def table(self):
        keys = [k for k, r in self.loaded.items() if r is not None]
        enc = np.zeros((len(keys), A), dtype=ENC_DTYPE)
        enc["weight"] = np.stack([self.loaded[k][0] for k in keys])
        enc["payoff"] = np.stack([self.loaded[k][1] for k in keys])
        enc["regret"], enc["visits"] = -3.0, 11
        return (np.array([k[0] for k in keys], np.uint64), np.array([k[1] for k in keys], np.uint32),
                np.array([k[2] for k in keys], np.uint64), enc)


class Model:
    """the model's answers for CASES and what it met on the way, computed once per process"""

    def __init__(self, salt=SALT):
        self.rows, self.trace, self.want = Rows(salt), [], []
        for name, h in CASES:
            self.rows.forbid = name == "absent"
            self.trace.append([])
            self.want.append(AM.corrections(h, self.rows, self.trace[-1]))
        self.rows.forbid = False
        self.table = self.rows.table()

    def of(self, name):
        return self.want[NAMES.index(name)]

    def nodes(self, kind, names=None):
        return [ev for i, t in enumerate(self.trace) for ev in t if ev["kind"] == kind and (names is None or NAMES[i] in names)]


_model = None


def model():
    global _model
    if _model is None:
        _model = Model()
    return _model


def placement(past, present, choices):
    """slot and home slot of every key after rp_nlhe_import into an empty table (insertion in order, linear probing)"""
    taken, slot, home = set(), [], []
    for p, q, c in zip(past, present, choices):
        h = PM.key_hash(int(p), int(c), int(q)) & (SLOTS - 1)
        s = h
        while s in taken:
            s = (s + 1) & (SLOTS - 1)
        taken.add(s)
        slot.append(s)
        home.append(h)
    return np.array(slot), np.array(home)

"""The batches of hands the match tests share (helper, no tests), the two blueprints they are played against, and the model's answers
with their trace.  tests/test_nlhe_match_model.py asserts on the CPU that every case the kernel has to get right occurs in them;
tests/test_gpu_nlhe_match.py compares rp_nlhe_match with the model on them.

The blueprints are decided key by key as the model asks, by a hash of the key and the table's salt: about three infosets in four get a
row, until the table's 2^10 slots are nearly used; the weights come from a small set, so that equal maxima are common (Dirac's tie).
Seat 0 reads table 0, seat 1 table 1.  SEED, the ids and LONG_ID were found by search with the model; the CPU test asserts what the
search was for."""
import itertools

import numpy as np

import nlhe_match_model as MM
import nlhe_policy_model as PM
from robopoker_amd.nlhe import A, ENC_DTYPE, AivatHand

CAP_LOG2 = 10
SLOTS = 1 << CAP_LOG2
SEED = 1
WEIGHTS = np.array([0.0, 1.0, 1.0, 3.0, 1e-39, 3.0, 0.5, 1e12], np.float32)  # 1e-39 is subnormal; 1.0 and 3.0 twice: ties
AGENTS = ("blueprint", "dirac", "fish")
# the hand of two fish that raise the minimum thirteen times before the flop: decisions 0..12 of this id all pick option 0 of 3
LONG_ID = 2121854


class Rows:
    """one blueprint, as the model reads it"""

    def __init__(self, salt):
        self.loaded, self.payoff, self.n_rows, self.salt = {}, {}, 0, salt

    def get(self, key):
        if key not in self.loaded:
            h = PM.key_hash(key[0] ^ self.salt, key[2], key[1])
            row = None
            if h % 4 != 0 and self.n_rows < SLOTS - 64:
                self.n_rows += 1
                row = WEIGHTS[[(h >> (8 + 3 * a)) & 7 for a in range(A)]].copy()
                row[PM.nch(key[2]):] = 7.0  # garbage past the infoset's actions
                self.payoff[key] = np.array([((h >> (32 + 3 * a)) & 7) - 3.5 for a in range(A)], np.float32)  # what AIVAT reads
            self.loaded[key] = row
        return self.loaded[key]

    def table(self):
        keys = [k for k, r in self.loaded.items() if r is not None]
        enc = np.zeros((len(keys), A), dtype=ENC_DTYPE)
        enc["weight"] = np.stack([self.loaded[k] for k in keys])
        enc["payoff"] = np.stack([self.payoff[k] for k in keys])
        enc["regret"], enc["visits"] = -3.0, 11
        return (np.array([k[0] for k in keys], np.uint64), np.array([k[1] for k in keys], np.uint32),
                np.array([k[2] for k in keys], np.uint64), enc)


def _configs():
    """(name, n, Args, one table for both seats)"""
    main = dict(seed=SEED, first_id=1001, dealer=2, mirror=True)  # an odd first id: hand 0 is the second of its pair
    out = [("main", 65, MM.Args(**main), False), ("main snap", 65, MM.Args(snap=True, **main), False),
           ("main hero 1", 65, MM.Args(hero=1, **main), False), ("main one table", 65, MM.Args(**main), True),
           ("pipeline", 65, MM.Args(seed=SEED, first_id=1001, dealer=0, board_mode=1), False),
           ("long street", 3, MM.Args(seed=SEED, first_id=LONG_ID - 1, agents=("fish", "fish"), dealer=0), False)]
    # each agent kind on either seat, both snap modes, mirror on and off; short stacks with the mirror: all-ins before the river
    for (a0, a1), snap, mirror in itertools.product(itertools.product(AGENTS, AGENTS), (False, True), (False, True)):
        args = MM.Args(seed=SEED + 1, first_id=2000, agents=(a0, a1), snap=snap, mirror=mirror, dealer=1 if mirror else 2,
                       stacks=(40, 25) if mirror else (0, 0), hero=int(snap), board_mode=int(mirror))
        out.append((f"{a0} {a1} snap {int(snap)} mirror {int(mirror)}", 17, args, False))
    return out


CONFIGS = _configs()
NAMES = [c[0] for c in CONFIGS]


def pack(hands):
    """the model's hands as the records the library writes"""
    return AivatHand.pack([AivatHand(w["holes"], w["draws"], w["plays"], seat=w["seat"], stacks=w["stacks"], dealer=w["dealer"],
                                     board_mode=w["board_mode"]) for w in hands])


class Model:
    """the model's answers for CONFIGS and what it met on the way, computed once per process"""

    def __init__(self):
        self.rows = (Rows(1), Rows(2))
        self.want, self.trace = {}, {}
        for name, n, args, one in CONFIGS:
            self.trace[name] = []
            self.want[name] = MM.match(n, args, (self.rows[0], self.rows[0]) if one else self.rows, trace=self.trace[name])
        self.tables = [r.table() for r in self.rows]

    def records(self, name):
        return pack(self.want[name])

    def column(self, name, field, dtype):
        return np.array([w[field] for w in self.want[name]], dtype)


_model = None


def model():
    global _model
    if _model is None:
        _model = Model()
    return _model

"""The batches of hands the search-match tests share (helper, no tests), the two blueprints they are played against, and the model's
answers with every search decision traced.  tests/test_nlhe_search_model.py asserts on the CPU that every case the kernels have to get
right occurs in them; tests/test_gpu_nlhe_search_match.py compares rp_nlhe_search_match with the model on them.

The blueprints are nlhe_match_cases.Rows — decided key by key as the model asks, by a hash of the key and the table's salt — with the
whole Encounter a solver warm-starts from and without that module's cap of 960 rows (a solve asks for every infoset of its tree; the
table is sized from what was asked).  Seat 0 reads table 0, seat 1 table 1.  Batches are tiny — 9 hands, 2 or 3 iterations, one
rollout, stacks (40, 25) so that the trees stay under RP_NLHE_DEPTH_MAX_NODES — and visit_threshold is 2, so that the blend moves the
policy.  The seeds and first ids were found by search with the model; the CPU test asserts what the search was for.  The model's
answers take about 12 s to compute.

No batch here holds RP_SEARCH_FALLBACK_SOLVE (a solve refused after a belief that was not): tests/test_gpu_nlhe_search_chunks.py pins
it on lookup-table encoders; what a search on the hash encoder met is written in tests/test_nlhe_search_model.py::test_every_case_occurs."""
import numpy as np

import nlhe_depth_model as DM
import nlhe_match_cases as K
import nlhe_match_model as MM
import nlhe_policy_model as PM
import nlhe_search_model as XM
from robopoker_amd.nlhe import A, SEARCH_STEP_DTYPE, Recall

EPOCH = 3  # what the tables are loaded with: the solver's warm start reads it
STEPS_CAP = 6
SEED, SEARCH_SEED = 7, 0x5EA2C4
SHORT = (40, 25)


class Rows(K.Rows):
    """nlhe_match_cases.Rows as a solver reads it: enc(key) is the row table() exports"""

    def get(self, key):
        if key not in self.loaded:
            h = PM.key_hash(key[0] ^ self.salt, key[2], key[1])
            row = None
            if h % 4 != 0:
                self.n_rows += 1
                row = K.WEIGHTS[[(h >> (8 + 3 * a)) & 7 for a in range(A)]].copy()
                row[PM.nch(key[2]):] = 7.0  # garbage past the infoset's actions
                self.payoff[key] = np.array([((h >> (32 + 3 * a)) & 7) - 3.5 for a in range(A)], np.float32)
            self.loaded[key] = row
        return self.loaded[key]

    def enc(self, key):
        w = self.get(key)
        if w is None:
            return None
        row = np.zeros(A, DM.ENC)
        row["weight"], row["payoff"], row["regret"], row["visits"] = w, self.payoff[key], -3.0, 11
        return row


def _configs():
    """(name, n, match Args, SearchArgs, one table for both seats)"""
    solve = dict(iterations=2, rollouts=1, visit_threshold=2, steps_cap=STEPS_CAP, search_seed=SEARCH_SEED)
    base = dict(seed=SEED, stacks=SHORT)
    both = dict(search=("world", "world"))
    return [
        ("world blueprint", 9, MM.Args(first_id=100, mirror=True, dealer=2, snap=True, **base), XM.SearchArgs(search=("world", "none"), **solve), False),
        ("fish dirac world", 9, MM.Args(first_id=58, agents=("fish", "dirac"), dealer=2, hero=1, **base),
         XM.SearchArgs(search=("none", "world"), **dict(solve, iterations=3)), False),
        ("both", 9, MM.Args(first_id=300, dealer=2, snap=True, **base), XM.SearchArgs(**both, **solve), False),
        ("both one table", 9, MM.Args(first_id=300, dealer=2, snap=True, **base), XM.SearchArgs(**both, **solve), True),
        ("world fish", 9, MM.Args(first_id=400, agents=("blueprint", "fish"), dealer=1, **base), XM.SearchArgs(search=("world", "none"), **solve), False),
        ("origin", 9, MM.Args(first_id=158, dealer=0, snap=True, **base), XM.SearchArgs(search=("world", "none"), origin_mode=1, **solve), False),
        ("deep", 3, MM.Args(first_id=600, seed=SEED, dealer=0, snap=True), XM.SearchArgs(search=("world", "world"), **solve), False),
    ]


CONFIGS = _configs()
NAMES = [c[0] for c in CONFIGS]
SEARCH_NAMES = NAMES


def config(name):
    return CONFIGS[NAMES.index(name)]


def pack_steps(hands, cap=STEPS_CAP):
    """the model's traced decisions as the records the library writes: [n][cap]"""
    out = np.zeros((len(hands), cap), SEARCH_STEP_DTYPE)
    for i, w in enumerate(hands):
        for k, s in enumerate(w["steps"][:cap]):
            r = out[i, k]
            r["solve_id"], r["decision"], r["seat"], r["edge"], r["fallback"], r["belief_status"] = (
                s["solve_id"], s["decision"], s["seat"], s["edge"], s["fallback"], s["belief_status"])
            r["bp"][: len(s["bp"])] = s["bp"]
            r["p"][: len(s["p"])] = s["p"]
            if s["recall"] is not None:
                r["recall"] = Recall.pack(s["recall"])[0]
                res = s["result"]
                for f in ("past", "choices", "present", "n_actions", "status", "regret", "sum_regret", "iterations", "n_rows", "nodes", "infosets",
                          "frontiers", "rollouts", "attempts", "fallbacks"):
                    r["result"][f] = res[f]
                r["result"]["refined"], r["result"]["visits"], r["result"]["drawn"] = res["refined"], res["visits"], res["drawn"]
    return out


class Model:
    """the model's answers for CONFIGS, computed once per process"""

    def __init__(self):
        self.rows = (Rows(1), Rows(2))
        self.want = {}
        for name, n, args, sargs, one in CONFIGS:
            self.want[name] = XM.match(n, args, sargs, (self.rows[0], self.rows[0]) if one else self.rows, EPOCH)
        self.tables = [r.table() for r in self.rows]
        self.cap_log2 = max((2 * t[0].size).bit_length() for t in self.tables)

    def records(self, name):
        return K.pack(self.want[name])

    def column(self, name, field, dtype):
        return np.array([w[field] for w in self.want[name]], dtype)

    def steps(self, name):
        return pack_steps(self.want[name])

    def all_steps(self, name):
        return [s for w in self.want[name] for s in w["steps"]]


_model = None


def model():
    global _model
    if _model is None:
        _model = Model()
    return _model

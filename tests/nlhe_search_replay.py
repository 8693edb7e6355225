"""The replay model of the search match (helper, no tests): nlhe_search_model.play's own hand loop — the deal, the witness, history(),
the key, the blueprint's distribution, blend, sample / argmax, the LENGTH / CAP / BELIEF / SOLVE / KEY order and the counters — with
ONE thing taken from the library: the belief and the harvest of a search decision, asked of the searching seat's handle through the two
public calls, NlheSolver.belief(recall) and NlheSolver.subgame_solve(entry, belief, origin, .., seed=search_seed, first_id=solve_id).
The recall and the entry are built here, from the model's witness, as nlhe_search_model.search_decision builds them.  Those two calls
are pinned against their own CPU models (tests/test_gpu_nlhe_world.py, tests/test_gpu_nlhe_subgame.py), and the header promises that a
step of rp_nlhe_search_match equals them bit for bit: a thousand hands are compared against a composition of independently verified
parts, where solving their three thousand subgames in Python (about 0.2 s each) is out of the question.

Hands are played in model ROUNDS, which are the library's: a hand stops at its first decision whose solve is not yet known and hands
back a request; the round's requests are answered seat by seat; the unfinished hands are replayed from their start, finished hands are
kept.  The k-th solve of a hand is asked for in round k of its chunk, so `rounds` also says how many requests of either seat
k_nl_search_compact has to place in a round.  One belief call per seat answers a round.  rp_nlhe_subgame_solve numbers the solves of
a call first_id, first_id + 1, ..: a round's solve ids (hand_id * 256 + decision) are never consecutive, so every solve is a call.

Table: the blueprint as the DEVICE holds it — get(key) answers from exactly the rows that were loaded into the handle, None for every
other key (nlhe_search_cases.Rows would invent a row by its hash that the device does not have)."""
import numpy as np

import nlhe_search_model as XM
from robopoker_amd.nlhe import Frontier, Recall


class Table:
    def __init__(self, table):
        past, present, choices, enc = table
        self.rows = {(int(p), int(q), int(c)): enc["weight"][i].copy() for i, (p, q, c) in enumerate(zip(past, present, choices))}

    def get(self, key):
        return self.rows.get(key)


class Passive:
    """The blueprints of the chunk-sized batch, decided key by key as the hands ask (seat 0's and seat 1's):
    every key nlhe_search_cases' own blueprints decided stays as decided — the nine hands of "both" play as they do there — and a PREFLOP
    key they never met gets a row that calls or checks 64 times as often as it takes any other edge.  Without those rows a blueprint
    that is uniform where it has no row folds two hands in three before the flop, and no round asks for more than 205 + 119 solves.
    The street of a key is the one its bucket states: nlhe_range_model._bucket answers street << 8 | bucket."""

    def __init__(self, bases):
        self.bases, self.extra = bases, ({}, {})

    def seat(self, s):
        return _PassiveSeat(self, s)

    def tables(self):
        """what to load: the bases' rows and the passive ones, (past, present, choices, Encounters) per seat"""
        out = []
        for base, extra in zip(self.bases, self.extra):
            past, present, choices, enc = base.table()
            more = np.zeros((len(extra), enc.shape[1]), enc.dtype)
            more["weight"], more["regret"], more["visits"] = np.stack(list(extra.values())), -3.0, 11
            keys = list(extra)
            out.append((np.concatenate([past, np.array([k[0] for k in keys], np.uint64)]), np.concatenate([present, np.array([k[1] for k in keys], np.uint32)]),
                        np.concatenate([choices, np.array([k[2] for k in keys], np.uint64)]), np.concatenate([enc, more])))
        return out


class _PassiveSeat:
    def __init__(self, both, s):
        self.base, self.extra = both.bases[s], both.extra[s]

    def get(self, key):
        if key in self.base.loaded:
            return self.base.loaded[key]
        if key not in self.extra and key[1] >> 8 == 0:
            n = XM.PM.nch(key[2])
            row = np.full(XM.PM.A, 7.0, np.float32)  # garbage past the infoset's actions
            row[:n] = [8.0 if int(e) in (XM.ON.E_CHECK, XM.ON.E_CALL) else 0.125 for e in XM.PM.edges(key[2])[:n]]
            self.extra[key] = row
        return self.extra.get(key)


class Pending(Exception):
    """a hand has met a search decision whose solve is not known yet"""

    def __init__(self, request):
        Exception.__init__(self)
        self.request = request


class Replay:
    """solvers: the handles of seat 0 and seat 1 (None: no solve is ever answered, only the first round is played, which needs
    no device); rows: the blueprint of either seat, a Table of what its handle was loaded with"""

    def __init__(self, solvers, rows, args, sargs, epoch=0, bucket=XM.RM._bucket):
        self.solvers, self.rows, self.args, self.sargs, self.epoch, self.bucket = solvers, tuple(rows), args, sargs, epoch, bucket
        self.known = {}  # solve_id -> (the belief's status, the SUBGAME_RESULT_DTYPE record)
        self.rounds = []  # [round] -> [(hand index, seat)] of the round's requests
        self.calls = 0

    def decision(self, sargs, hand_id, decision, turn, witness, stacks, dealer, dealt, hole, rows, bp_epoch, key, slots, bp):
        """nlhe_search_model.search_decision with the belief and the harvest looked up"""
        edges = witness.history()
        solve_id = (hand_id * 256 + (decision & 255)) & XM.RO.M64
        recall = Recall(turn, hole, dealt, edges, stacks, dealer)
        if solve_id not in self.known:
            holes = [0, 0]
            holes[turn] = hole
            entry = Frontier(holes, turn, dealt, edges, witness.subgame()[:XM.MAX_PREFIX], stacks, dealer)
            raise Pending(dict(solve_id=solve_id, seat=turn, recall=recall, entry=entry, origin=len(dealt) - 1 if sargs.origin_mode else None))
        status, res = self.known[solve_id]
        if status != XM.RM.OK:
            code = XM.BELIEF
        elif int(res["status"]) != XM.RM.OK:
            code = XM.SOLVE
        elif (int(res["past"]), int(res["present"]), int(res["choices"])) != key:
            code = XM.KEY
        else:
            code = XM.SOLVED
        p = XM.blend(res["refined"], res["visits"], bp, slots, sargs.visit_threshold) if code == XM.SOLVED else list(bp)
        return dict(solve_id=solve_id, recall=recall, result=res, belief_status=status, bp=list(bp), p=p, seat=turn, decision=decision, fallback=code)

    def answer(self, requests):
        a = self.sargs
        for seat in (0, 1):
            mine = [r for r in requests if r["seat"] == seat]
            if not mine:
                continue
            s = self.solvers[seat]
            bel = s.belief(Recall.pack([r["recall"] for r in mine]))
            entries = Frontier.pack([r["entry"] for r in mine])
            self.calls += 1
            for j, r in enumerate(mine):
                res, _, _ = s.subgame_solve(entries[j: j + 1], (bel["hole_world"][j], bel["weights"][j]), r["origin"], a.iterations, a.rollouts,
                                            a.bias, a.prior, a.search_seed, r["solve_id"])
                self.known[r["solve_id"]] = (int(bel["status"][j]), res[0].copy())
                self.calls += 1

    def match(self, n):
        """-> nlhe_search_model.match's list of hands (None for a hand left waiting where there are no solvers)"""
        out, waiting, self.rounds = [None] * n, list(range(n)), []
        model, XM.search_decision = XM.search_decision, self.decision
        try:
            while waiting:
                requests, still = [], []
                for i in waiting:
                    try:
                        out[i] = XM.play(self.args.first_id + i, self.args, self.sargs, self.rows, self.epoch, self.bucket)
                    except Pending as p:
                        requests.append(p.request)
                        still.append(i)
                if requests:
                    self.rounds.append([(i, r["seat"]) for i, r in zip(still, requests)])
                if self.solvers is None:
                    break
                self.answer(requests)
                waiting = still
        finally:
            XM.search_decision = model
        return out

    def counts(self, lo, hi):
        """[round] -> (seat 0's requests, seat 1's) among the hands lo <= i < hi: what the chunk [lo, hi) compacts in that round"""
        return [tuple(sum(1 for i, s in r if lo <= i < hi and s == seat) for seat in (0, 1)) for r in self.rounds]


CHUNK = 1024  # NSM_CHUNK (csrc/nlmc_search.hpp): hands in flight
BIG_N = CHUNK + 64 + 1  # a chunk, and a wavefront and one hand of the next
BIG_CAP = 2  # the big batch's steps_cap, below its hands' most search decisions: parked and resumed hands go on untraced
_big = None


def big_batch():
    """The batch that fills a chunk and enters a second — "both" of nlhe_search_cases (first_id 300: its hands [0, 9) are that
    config's own, stacks (40, 25), both seats searching on two tables) from BIG_N hands on, steps_cap BIG_CAP, against the Passive
    blueprints — computed once per process, on the CPU: dict(args, sargs, tables: what to load into the two handles; first: the
    requests of seat 0 and seat 1 in the first round of the first chunk, which needs no solve to be known)"""
    global _big
    if _big is None:
        import nlhe_search_cases as SC

        _, _, args, sargs, _ = SC.config("both")
        sargs = XM.SearchArgs(**dict(sargs.kwargs(), steps_cap=BIG_CAP))
        blueprints = Passive(SC.model().rows)
        first = Replay(None, (blueprints.seat(0), blueprints.seat(1)), args, sargs, SC.EPOCH)
        first.match(BIG_N)
        tables = blueprints.tables()
        _big = dict(args=args, sargs=sargs, tables=tables, first=first.counts(0, CHUNK)[0],
                    cap_log2=max((2 * t[0].size).bit_length() for t in tables))
    return _big

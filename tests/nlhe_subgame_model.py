"""The model the safe-subgame tests compare against (helper, no tests): rp_nlhe_subgame_solve (include/rp_mi355x.h) by the NAIVE
algorithm of the reference — SubGameSolver::step / harvest (subgame/src/solver.rs:146-229) over SubGameEncoder (subgame/src/encoder.rs),
WorldProfile (world/profile.rs) over DepthView, and NlheEncoder::restrict for the deal of every iteration.

It is nlhe_depth_model's Solve with three things added, none of them by editing that module: before every tree a deal from
nlhe_world_model.restrict_one (the belief handed in as data: the world of every candidate hole and four weights), the world of that deal
as the last member of every infoset of the tree — an infoset is (kind, past, present, choices, world), so that everything
nlhe_depth_model reads by position stays where it is; rows are exported in (world, kind, past, present, choices) order — and the harvest
as the three folds over the worlds, restated literally.  The kernel (robopoker_amd/csrc/nlmc_subgame.hpp) finds the first accepted attempt
with all its lanes, keeps the world in two bits of a row's key and orders the regret fold by a table, so that this checks them."""
from __future__ import annotations

import ctypes as C

import numpy as np

import nlhe_depth_model as DM
import nlhe_rollout_model as FM
import nlhe_world_model as WM
import oracle_nlhe as ON
from robopoker_amd.nlhe import Frontier, Recall

F = DM.F
PM = DM.PM
EPS, M64, A, OK = DM.EPS, DM.M64, DM.A, DM.OK
GAME, PICK = DM.GAME, DM.PICK
WORLDS, WORLD_NONE, MAX_REJECTIONS = WM.WORLDS, WM.WORLD_NONE, WM.MAX_REJECTIONS
MAX_ITERATIONS = DM.MAX_ITERATIONS
MAX_ROWS = 2048  # RP_NLHE_SUBGAME_MAX_ROWS
ORIGIN_NONE = 126  # RP_NLHE_SUBGAME_ORIGIN_NONE
NEVER = 4  # no street lies beyond it: DepthGame::at_frontier with origin = None
Malformed = DM.Malformed
fold = DM.fold


def free_cards(hole: int, board: int):
    return [c for c in range(52) if not (hole | board) >> c & 1]


def candidate(free, hole: int) -> int:
    """the index k_nl_world gives a hole: hi (hi - 1) / 2 + lo over the positions of its cards among the free cards"""
    lo, hi = sorted(free.index(c) for c in range(52) if hole >> c & 1)
    return hi * (hi - 1) // 2 + lo


def edge_order(edge: int):
    """the derived Ord of kicker::Edge (kicker/src/edge.rs:18-27): Draw < Fold < Check < Call < Open(n) < Raise(Odds(n, d)) < Shove, the
    payloads compared as they are written — Odds lexicographically by (n, d), not by value"""
    if edge in (ON.E_DRAW, ON.E_FOLD, ON.E_CHECK, ON.E_CALL):
        return (edge - 1,)
    if edge == ON.E_SHOVE:
        return (6,)
    return (4, ON.OPENS[edge - 6]) if edge < 10 else (5,) + tuple(ON.RAISES[edge - 10])


class Profile(DM.Profile):
    """WorldProfile over DepthView: the local dict keyed with the world, every read that misses it answered for the untagged info"""

    def view(self, info, a, field):
        return DM.Profile.view(self, info[:4], a, field)

    def sorted_infos(self):
        return sorted(self.local, key=lambda i: (i[4],) + i[:4])


def dummy_hole(entry) -> int:
    """two cards no field of the record holds: the other seat's hole is not an input, the record is validated without it"""
    taken = entry.holes[entry.internal]
    for d in entry.draws:
        taken |= d
    low = [c for c in range(52) if not taken >> c & 1][:2]
    return 1 << low[0] | 1 << low[1]


def with_hole(entry, hole: int):
    holes = list(entry.holes)
    holes[1 - entry.internal] = hole
    return Frontier(holes, entry.internal, entry.draws, entry.edges, entry.prefix, entry.stacks, entry.dealer)


class Solve(DM.Solve):
    """one solve: entry = a Frontier record whose hole for the seat opposite `internal` is not read; hole_world uint8[1326], weights
    float32[4] = the belief; origin None = ORIGIN_NONE.  force: a hole every iteration deals instead of the restricted one (tests only)"""

    def __init__(self, entry, hole_world, weights, origin, bp, index=0, hyper=None, bp_epoch=0, rollouts=16, bias=5.0, prior=float(1 << 14),
                 seed=0, first_id=0, force=None):
        if entry.internal > 1:  # the seat is read before anything else can be
            raise Malformed(FM.SEAT)
        self.origin_none = origin is None
        DM.Solve.__init__(self, with_hole(entry, dummy_hole(entry)), NEVER if origin is None else origin, bp, index, hyper, bp_epoch, rollouts,
                          bias, prior, seed, first_id)
        self.profile = Profile(bp, hyper or DM.Hyper(), prior, bp_epoch)
        self.base, self.force = self.entry, force
        self.weights = np.asarray(weights, F)
        if not np.isfinite(self.weights).all() or (self.weights < 0).any():
            raise Malformed(FM.CARDS)
        hw = np.asarray(hole_world, np.uint8)
        self.hole_world = np.where(hw < WORLDS, hw, WORLD_NONE).astype(np.uint8)  # the belief is data: 4 .. 254 reads as no world
        self.recall = Recall(entry.internal, entry.holes[entry.internal], entry.draws, entry.edges, entry.stacks, entry.dealer)
        self.free = free_cards(self.recall.hole, self.game.board)
        self.count = len(self.free) * (len(self.free) - 1) // 2
        self.world, self.deals = None, []  # (hole, world, attempts) of every iteration
        self.drawn, self.attempts, self.fallbacks = [0] * WORLDS, 0, 0
        self._cache = {}

    def info_of(self, node):
        info = DM.Solve.info_of(self, node)
        return None if info is None else info + (self.world,)

    def deal(self):
        """NlheEncoder::restrict for iteration t: deal t of `recall` among 4096"""
        deal = WM.Deal(self.seed, WM.deal_id(self.id, 0, MAX_ITERATIONS, self.profile.t))
        bel = {"weights": self.weights, "world": self.hole_world}
        by_candidate = lambda street, hole, board: candidate(self.free, hole)  # noqa: E731
        hole, world, attempts = WM.restrict_one(self.recall, bel, WORLD_NONE, deal, by_candidate, self._cache)
        return (self.force if self.force is not None else hole), world, attempts

    def step(self):
        hole, world, attempts = self.deal()
        self.deals.append((hole, world, attempts))
        self.drawn[world] += 1
        self.attempts += attempts
        self.fallbacks += attempts == MAX_REJECTIONS
        self.world = world
        self.entry = with_hole(self.base, hole)
        self.game = FM._copy(self.game)
        self.game.seats[1 - self.internal].cards = hole
        depth_cap, DM.MAX_ROWS = DM.MAX_ROWS, MAX_ROWS  # the one number of nlhe_depth_model's step that differs here
        try:
            DM.Solve.step(self)
        finally:
            DM.MAX_ROWS = depth_cap

    def harvest(self):
        """Harvest::harvest (subgame/src/solver.rs:184-229) at Game(key of the entry state), the rows, the counters"""
        p = self.profile
        out = failed(OK)
        out.update(sum_regret=p.sum_regret(), iterations=p.t, drawn=list(self.drawn), attempts=self.attempts, fallbacks=self.fallbacks,
                   deals=list(self.deals), **self.counters)
        turn = DM.inner_turn(self.game)
        if turn >= 0:
            key = FM.key_at(self.game, list(self.entry.prefix), turn)  # the entry state as the last iteration dealt it
            n = PM.nch(key[2])
            edges = [int(e) for e in PM.edges(key[2])[:n]]
            depth = (GAME,) + key
            out.update(past=key[0], present=key[1], choices=key[2], n_actions=n)
            refined = {}
            for w in range(WORLDS):
                for e, pr in zip(edges, p.iterated(depth + (w,))):
                    refined[e] = F(refined.get(e, F(0.0)) + F(pr / F(WORLDS)))
            visits = {e: sum(int(p.cum(depth + (w,), edges.index(e), "visits")) for w in range(WORLDS)) & 0xFFFFFFFF for e in refined}
            regret = fold(np.fmax(p.cum(depth + (w,), edges.index(e), "regret"), F(0.0)) for e in sorted(refined, key=edge_order)
                          for w in range(WORLDS))
            out["refined"][:n] = [refined[e] for e in edges]
            out["visits"][:n] = [visits[e] for e in edges]
            out["regret"] = regret
        rows = []
        for info in p.sorted_infos():
            enc = np.zeros(A, dtype=DM.ENC)
            for a, e in p.local[info].items():
                enc[a] = (e["weight"], e["regret"], e["payoff"], e["visits"])
            rows.append((info[4], info[0], p.n(info), info[1], info[2], info[3], enc))  # world, kind, n_actions, past, present, choices
        out["rows"], out["n_rows"] = rows, len(rows)
        return out


def failed(status):
    out = DM.failed(status)
    out.update(drawn=[0] * WORLDS, attempts=0, fallbacks=0, deals=[])
    return out


def solve(entry, hole_world, weights, origin, bp, index=0, iterations=1, keep=None, **kw):
    """one entry of a batch -> harvest dict; origin: None or ORIGIN_NONE = adapt_full as written, -1 .. 3 = with_origin"""
    try:
        if origin == ORIGIN_NONE:
            origin = None
        if origin is not None and not -1 <= origin <= 3:
            if entry.internal <= 1:
                FM.frontier_game(with_hole(entry, dummy_hole(entry)))  # the record's own status comes first
            raise Malformed(FM.SEAT)
        s = Solve(entry, hole_world, weights, origin, bp, index, **kw)
        if keep is not None:
            keep.append(s)
        for _ in range(iterations):
            s.step()
        return s.harvest()
    except Malformed as m:
        return failed(m.status)


def one_world(entry, world: int = 0):
    """a belief whose `world` holds every candidate hole with weight 1"""
    hole_world = np.full(WM.RM.MAX_HOLES, WORLD_NONE, np.uint8)
    g = FM.frontier_game(with_hole(entry, dummy_hole(entry)))
    n = len(free_cards(entry.holes[entry.internal], g.board))
    hole_world[: n * (n - 1) // 2] = world
    weights = np.zeros(WORLDS, F)
    weights[world] = 1.0
    return hole_world, weights

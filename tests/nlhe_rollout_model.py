"""The model the frontier-payoff tests compare against (helper, no tests): rp_nlhe_frontier_payoffs (include/rp_mi355x.h) by the NAIVE
algorithm of the reference (DepthSampler::payoffs, nlhe/src/solver.rs:39-67; NlheEncoder::biased_rollout / sample_biased,
nlhe/src/encoder.rs:70-147) — one game per rollout, played in Python over the CPU oracle's rules engine (ora_nlhe_from_start, apply,
actionize, snap, choices, info, payoff), bucketed with the oracle's isomorphism and hash encoder, the averaged policy from
nlhe_policy_model.distribution over a dict of rows, sample_biased in explicit numpy float32 steps.

The story is a plain list of every edge (prefix, then one per step) and is cut to its first 12 edges only where a key is formed;
the kernel (robopoker_amd/csrc/nlmc_frontier.hpp) keeps a few counters instead, so that this checks them.  The random numbers are
the library's counter contract restated on Python integers (include/rp_math.h: rp_node_hash, rp_u01, rp_pick_uniform)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import nlhe_policy_model as PM
import nlhe_range_model as RM
import oracle_nlhe as ON

F = np.float32
LEAVES, CELLS, MAX_PREFIX, MAX_ROLLOUTS = 4, 16, 12, 4096
MAX_STEPS = 12 * 32768  # NF_MAX_STEPS
M64 = PM.M64
OK, EDGE, ILLEGAL, LENGTH, CARDS, DRAW, SEAT, LOOKUP = range(8)  # rp_recall_status
Malformed = RM.Malformed


# ---- the counter contract ----
def node_hash(seed: int, epoch: int, tree: int, key: int) -> int:
    """rp_node_hash"""
    h = PM._mix64((seed + 0x9E3779B97F4A7C15) & M64)
    h = PM._mix64(h ^ ((epoch * 0xD1342543DE82EF95 + 0x632BE59BD9B4E019) & M64))
    h = PM._mix64(h ^ ((tree * 0xAF251AF3B0F025B5 + 0x2545F4914F6CDD1D) & M64))
    lo, hi, k = h & 0xFFFFFFFF, h >> 32, (key ^ (key >> 32)) & 0xFFFFFFFF
    x = lo ^ k
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    x = ((x ^ hi) * 0x9E3779B1) & 0xFFFFFFFF
    x ^= x >> 15
    return x << 32


def u01(h: int) -> np.float32:
    """rp_u01: the top 24 bits as a float in [0, 1)"""
    return F(F(h >> 40) * F(5.9604644775390625e-8))


def pick_uniform(h: int, n: int) -> int:
    """rp_pick_uniform"""
    return ((h >> 32) * n) >> 32


def rollout_id(first_id: int, i: int, k: int, j: int, rollouts: int, r: int) -> int:
    return ((((first_id + i) & M64) * CELLS + 4 * k + j) * rollouts + r) & M64


class Stream:
    """the draws of one rollout in consumption order; `used` keeps the counters handed out"""

    def __init__(self, seed: int, rid: int):
        self.seed, self.rid, self.c = seed, rid, 0

    def next(self) -> int:
        h = node_hash(self.seed, 0, self.rid, self.c)
        self.c += 1
        return h


# ---- sample_biased (encoder.rs:121-146) ----
def multiplier(continuation: int, edge: int, bias) -> np.float32:
    folded, aggro = edge == ON.E_FOLD, edge == ON.E_SHOVE or edge >= 6
    hit = (continuation == 1 and folded) or (continuation == 2 and not folded and not aggro) or (continuation == 3 and aggro)
    return F(bias) if hit else F(1.0)


def biased_weights(dist, edges, continuation: int, bias):
    return [F(F(p) * multiplier(continuation, int(e), bias)) for p, e in zip(dist, edges)]


def sample_biased(dist, edges, continuation: int, bias, u) -> int:
    """-> the slot sampled: dist float32[n], edges [n], u = the uniform draw"""
    with np.errstate(all="ignore"):
        w = biased_weights(dist, edges, continuation, bias)
        total = F(0.0)
        for x in w:
            total = F(total + x)
        threshold = F(F(u) * total)
        acc = F(0.0)
        for a, x in enumerate(w):
            acc = F(acc + x)
            if threshold < acc:
                return a
    return len(w) - 1


# ---- the frontier state ----
def validate(f):
    if len(f.edges) > RM.MAX_HISTORY or len(f.prefix) > MAX_PREFIX:
        raise Malformed(LENGTH)
    if f.internal > 1 or f.dealer > 1 or (tuple(f.stacks) != (0, 0) and min(f.stacks) <= 0):
        raise Malformed(SEAT)
    gone = 0
    for hole in f.holes:
        if hole & ~RM.FULL or RM.popcount(hole) != 2 or hole & gone:
            raise Malformed(CARDS)
        gone |= hole
    draws = list(f.draws) + [0] * (3 - len(f.draws))
    for s, d in enumerate(draws):
        if d == 0:
            continue
        if d & ~RM.FULL or RM.popcount(d) != (3 if s == 0 else 1) or d & gone or (s > 0 and draws[s - 1] == 0):
            raise Malformed(CARDS)
        gone |= d
    if any(e < 1 or e > 19 for e in tuple(f.edges) + tuple(f.prefix)):
        raise Malformed(EDGE)
    return draws


def frontier_game(f):
    """the state after f.edges, replayed as the ranges replay (NlheGame::apply with the frontier's draws), both seats holding cards"""
    draws = validate(f)
    g = RM._game(f, list(f.holes))
    for e in f.edges:
        RM._apply(g, e, draws)
    return g


def _copy(g):
    out = ON.GameStruct()
    C.memmove(C.byref(out), C.byref(g), C.sizeof(ON.GameStruct))
    return out


def deal(g, stream: Stream) -> int:
    """game.reveal(): one street, card by card — the pick-th lowest card of the deck, which then loses it"""
    taken = g.board | g.seats[0].cards | g.seats[1].cards
    deck = [c for c in range(52) if not taken >> c & 1]
    cards = 0
    for _ in range(3 if ON.lib().ora_nlhe_street(C.byref(g)) == 0 else 1):
        cards |= 1 << deck.pop(pick_uniform(stream.next(), len(deck)))
    return cards


def key_at(g, story, actor: int):
    """resume(story, game): (past, present, choices) from the first 12 edges of the story"""
    o = ON.lib()
    past, choices = C.c_uint64(), C.c_uint64()
    o.ora_nlhe_info(C.byref(g), ON.path_pack(list(story[:MAX_PREFIX])), C.byref(past), C.byref(choices))
    present = RM._bucket(o.ora_nlhe_street(C.byref(g)), g.seats[actor].cards, g.board)
    return past.value, present, choices.value


def rollout(game, prefix, internal: int, k: int, j: int, rows, bias, stream: Stream, used=None) -> int:
    """biased_rollout (encoder.rs:89-115) -> won of seat `internal`; used collects (key, found, story length) of every decision"""
    o = ON.lib()
    g = _copy(game)
    story = list(prefix)
    for _ in range(MAX_STEPS):
        turn = o.ora_nlhe_turn(C.byref(g))
        if turn == ON.TERMINAL:
            out = C.c_float()
            assert o.ora_nlhe_payoff(C.byref(g), internal, C.byref(out)) == 0
            return int(out.value)
        if turn == ON.CHANCE:
            story.append(ON.E_DRAW)
            assert o.ora_nlhe_apply(C.byref(g), C.byref(ON.ActionStruct(ON.DRAW, 0, deal(g, stream)))) == 0
            continue
        key = key_at(g, story, turn)
        n = PM.nch(key[2])
        if n == 0:
            raise Malformed(ILLEGAL)
        w = rows.get(key)
        if used is not None:
            used.append((key, w is not None, len(story)))
        dist = PM.distribution("averaged", np.zeros(PM.A, F) if w is None else w, n)[:n]
        edges = PM.edges(key[2])[:n]
        edge = int(edges[sample_biased(dist, edges, k if turn == internal else j, bias, u01(stream.next()))])
        action = o.ora_nlhe_snap(C.byref(g), o.ora_nlhe_actionize(C.byref(g), edge, 0))
        story.append(edge)
        if o.ora_nlhe_apply(C.byref(g), C.byref(action)):
            raise Malformed(ILLEGAL)
    raise Malformed(ILLEGAL)


def payoffs(f, rows, index: int, bias=5.0, rollouts=16, seed=0, first_id=0, used=None):
    """one frontier, the index-th of its batch -> (status, payoffs float32[4,4], won int16[16, rollouts])"""
    rollouts = max(rollouts, 1)
    pay, won = np.zeros((LEAVES, LEAVES), F), np.zeros((CELLS, rollouts), np.int16)
    try:
        game = frontier_game(f)
        for k in range(LEAVES):
            for j in range(LEAVES):
                total = F(0.0)
                for r in range(rollouts):
                    stream = Stream(seed, rollout_id(first_id, index, k, j, rollouts, r))
                    won[4 * k + j, r] = rollout(game, f.prefix, f.internal, k, j, rows, bias, stream, used)
                    total = F(total + F(won[4 * k + j, r]))
                pay[k, j] = F(total / F(rollouts))
    except Malformed as m:
        return m.status, np.zeros((LEAVES, LEAVES), F), np.zeros((CELLS, rollouts), np.int16)
    return OK, pay, won

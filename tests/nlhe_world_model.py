"""The model the subgame-world tests compare against (helper, no tests): rp_nlhe_partition / rp_nlhe_belief / rp_nlhe_restrict
(include/rp_mi355x.h) by the NAIVE algorithms of the reference — Partition::partition::<4> (subgame/src/world/partition.rs:26-52) as a
Python loop over np.float32 scalars and Python's stable sorted, Nlhe::setup (nlhe/src/solver.rs:129-136) over
nlhe_range_model.opponent_range, and NlheEncoder::restrict (nlhe/src/encoder.rs:148-186) as the sequential attempt loop.

The kernel (robopoker_amd/csrc/nlmc_world.hpp) ranks the buckets in parallel, keeps only where the scan advances, and decides an
attempt by one byte of a per-candidate table; this model sorts, walks the sorted list, and buckets every attempted hole again with the
oracle's isomorphism and encoder, so that it checks those shortcuts.  The random numbers are the library's counter contract as
nlhe_rollout_model restates it."""
from __future__ import annotations

import numpy as np

import nlhe_range_model as RM
import nlhe_rollout_model as FM

F = np.float32
WORLDS, MAX_REJECTIONS, WORLD_NONE, EPOCH = 4, 10000, 0xFF, 1
M64 = FM.M64


def partition(mass, seen):
    """-> (world uint8[256], weights float32[4], total float32)"""
    entries = [(b, F(mass[b])) for b in range(256) if seen[b]]  # the BTreeMap's order
    world, weights = np.full(256, WORLD_NONE, np.uint8), np.zeros(WORLDS, F)
    total = F(0.0)
    with np.errstate(all="ignore"):
        for _, m in entries:
            total = F(total + m)
        if total <= 0:
            for b, _ in entries:
                world[b] = 0
            weights[:] = F(1.0) / F(WORLDS)
            return world, weights, total
        ordered = sorted(entries, key=lambda e: -float(e[1]))  # descending, stable: equal masses keep ascending b
        segment = F(total / F(WORLDS))
        index, bucket, accumulated = 0, F(0.0), F(0.0)
        for b, m in ordered:
            bucket = F(bucket + m)
            accumulated = F(accumulated + m)
            world[b] = index
            if accumulated >= F(segment * F(index + 1)) and index < WORLDS - 1:
                weights[index] = F(bucket / total)
                index += 1
                bucket = F(0.0)
        weights[index] = F(bucket / total)
    return world, weights, total


def hash_bucket(street: int, hole: int, board: int) -> int:
    """the hash encoder's bucket index: the oracle's isomorphism and hash"""
    return RM._bucket(street, hole, board) & 255


def belief(r, rows, stream=None, bucket=hash_bucket):
    """-> dict(status, world uint8[256], weights float32[4], hole_world uint8[1326], total, count, mass, seen); bucket(street, hole,
    board) -> the bucket index, or None for a hole the encoder does not know (RP_RECALL_LOOKUP)"""
    status, holes, reach = stream if stream is not None else RM.reaches(r, "opponent", rows)
    mass, seen = np.zeros(256, F), np.zeros(256, bool)
    hole_bucket = []
    if status == RM.OK:
        street, board, _ = RM.board_of(r, RM.validate(r))
        hole_bucket = [bucket(street, int(h), board) for h in holes]
        if any(b is None for b in hole_bucket):
            status, hole_bucket = RM.LOOKUP, []
    for b, x in zip(hole_bucket, reach):
        mass[b] = F(mass[b] + x)
        seen[b] = True
    world, weights, total = partition(mass, seen)
    hole_world = np.full(RM.MAX_HOLES, WORLD_NONE, np.uint8)
    hole_world[: len(hole_bucket)] = [world[b] for b in hole_bucket]
    return dict(status=status, world=world, weights=weights, hole_world=hole_world, total=total, count=len(hole_bucket), mass=mass, seen=seen)


class Deal:
    """the draws of one deal: draw c = rp_node_hash(seed, 1, deal_id, c)"""

    def __init__(self, seed: int, deal_id: int):
        self.seed, self.deal_id = seed, deal_id & M64
        # a fallback deal takes 20 002 draws: everything of FM.node_hash that does not depend on c is kept, so that draw(c) finishes
        # from key 0's result (tests/test_nlhe_world_model.py holds draw(c) == FM.node_hash(seed, 1, deal_id, c))
        self._lo, self._hi = self._halves()

    def _halves(self):
        h = FM.PM._mix64((self.seed + 0x9E3779B97F4A7C15) & M64)
        h = FM.PM._mix64(h ^ ((EPOCH * 0xD1342543DE82EF95 + 0x632BE59BD9B4E019) & M64))
        h = FM.PM._mix64(h ^ ((self.deal_id * 0xAF251AF3B0F025B5 + 0x2545F4914F6CDD1D) & M64))
        return h & 0xFFFFFFFF, h >> 32

    def draw(self, c: int) -> int:
        x = self._lo ^ (c & 0xFFFFFFFF)
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & 0xFFFFFFFF
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & 0xFFFFFFFF
        x ^= x >> 16
        x = ((x ^ self._hi) * 0x9E3779B1) & 0xFFFFFFFF
        x ^= x >> 15
        return x << 32


def deal_id(first_id: int, r: int, deals: int, d: int) -> int:
    return (((first_id + r) & M64) * deals + d) & M64


def draw_world(weights, u) -> int:
    with np.errstate(all="ignore"):
        total = F(0.0)
        for w in weights:
            total = F(total + w)
        x = F(F(u) * total)
        acc = F(0.0)
        for k, w in enumerate(weights):
            acc = F(acc + w)
            if x < acc:
                return k
    nonzero = [k for k, w in enumerate(weights) if w != 0]
    return nonzero[-1] if nonzero else 0


def attempt(deal: Deal, a: int, free):
    """attempt a: the pick-th lowest free card, then the pick-th lowest of the rest -> the two cards"""
    rest = list(free)
    first = rest.pop(FM.pick_uniform(deal.draw(1 + 2 * a), len(rest)))
    second = rest.pop(FM.pick_uniform(deal.draw(2 + 2 * a), len(rest)))
    return first, second


def restrict_one(r, bel, request: int, deal: Deal, bucket=hash_bucket, cache=None):
    """one deal of a valid recall -> (hole, world_out, attempts); cache: {hole: world} across the deals of one recall (a memo of the
    per-hole bucketing below, not the belief's candidate table)"""
    if request != WORLD_NONE and request >= WORLDS:
        return 0, WORLD_NONE, 0
    world = request if request != WORLD_NONE else draw_world(bel["weights"], FM.u01(deal.draw(0)))
    street, board, _ = RM.board_of(r, RM.validate(r))
    free = [c for c in range(52) if not (r.hole | board) >> c & 1]
    cache = {} if cache is None else cache
    for a in range(MAX_REJECTIONS):
        c0, c1 = attempt(deal, a, free)
        hole = 1 << c0 | 1 << c1
        if hole not in cache:
            cache[hole] = int(bel["world"][bucket(street, hole, board)])  # Belief::remember: the secret's world
        if cache[hole] == world:
            return hole, world, a
    c0, c1 = attempt(deal, MAX_REJECTIONS, free)
    return 1 << c0 | 1 << c1, world, MAX_REJECTIONS


def restrict(r, bel, index: int, deals: int, worlds=None, seed=0, first_id=0, bucket=hash_bucket):
    """one recall, the index-th of its batch -> (holes uint64[deals], world_out uint8[deals], attempts uint16[deals])"""
    holes, out, attempts = np.zeros(deals, np.uint64), np.full(deals, WORLD_NONE, np.uint8), np.zeros(deals, np.uint16)
    if bel["status"] != RM.OK:
        return holes, out, attempts
    cache = {}
    for d in range(deals):
        request = WORLD_NONE if worlds is None else int(worlds[d])
        holes[d], out[d], attempts[d] = restrict_one(r, bel, request, Deal(seed, deal_id(first_id, index, deals, d)), bucket, cache)
    return holes, out, attempts

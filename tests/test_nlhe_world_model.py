"""Pins tests/nlhe_world_model.py, the naive model the GPU world tests (tests/test_gpu_nlhe_world.py) compare against, and the new
symbols of the C ABI (rp_nlhe_partition, rp_nlhe_belief, rp_nlhe_restrict and their _device forms).  No GPU."""
import os
import re

import numpy as np

import nlhe_range_model as RM
import nlhe_rollout_model as FM
import nlhe_world_model as WM
import oracle_nlhe as ON
from robopoker_amd import _lib
from robopoker_amd import nlhe as N
from robopoker_amd.nlhe import Recall

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = WM.WORLD_NONE


def cards(*cs):
    return sum(1 << c for c in cs)


HOLE, FLOP = cards(51, 50), cards(3, 17, 30)


def row(masses, at=None):
    """(mass[256], seen[256]) with the given masses at buckets `at` (default 0, 1, ...)"""
    mass, seen = np.zeros(256, F), np.zeros(256, bool)
    for b, m in zip(at if at is not None else range(len(masses)), masses):
        mass[b], seen[b] = m, True
    return mass, seen


def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def test_hand_rows():
    world, weights, total = WM.partition(*row([4, 3, 2, 1]))
    # total 10, segment 2.5: 4 >= 2.5, 7 >= 5, 9 >= 7.5, and the last entry is what is left
    assert list(world[:4]) == [0, 1, 2, 3] and (world[4:] == NONE).all() and total == 10
    assert np.array_equal(bits(weights), bits([F(4) / F(10), F(3) / F(10), F(2) / F(10), F(1) / F(10)]))
    world, weights, _ = WM.partition(*row([10, 1]))
    # segment 2.75: 10 >= 2.75 closes world 0, and one entry advances at most once; 11 >= 5.5 closes world 1; nothing is left for 2
    assert list(world[:2]) == [0, 1] and np.array_equal(bits(weights), bits([F(10) / F(11), F(1) / F(11), 0, 0]))
    # the order is by mass, not by bucket: the same masses on other buckets, ascending
    world, weights, _ = WM.partition(*row([1, 2, 3, 4], at=[7, 40, 41, 255]))
    assert [world[b] for b in (7, 40, 41, 255)] == [3, 2, 1, 0] and np.array_equal(bits(weights), bits([F(0.4), F(0.3), F(0.2), F(0.1)]))


def test_equal_masses_over_all_buckets():
    world, weights, total = WM.partition(np.ones(256, F), np.ones(256, bool))
    assert total == 256 and [int((world == w).sum()) for w in range(4)] == [64] * 4
    assert list(world) == sorted(world)  # stable: ties keep ascending b
    assert np.array_equal(bits(weights), bits([0.25] * 4))


def test_zero_total_and_empty_rows():
    world, weights, total = WM.partition(*row([0, 0, 0], at=[3, 9, 200]))
    assert total == 0 and [world[b] for b in (3, 9, 200)] == [0, 0, 0] and (world != NONE).sum() == 3
    assert np.array_equal(bits(weights), bits([0.25] * 4))
    world, weights, total = WM.partition(np.zeros(256, F), np.zeros(256, bool))
    assert total == 0 and (world == NONE).all() and np.array_equal(bits(weights), bits([0.25] * 4))
    # a mass where seen is 0 is no entry
    mass, seen = row([5, 1])
    mass[77] = 100
    assert WM.partition(mass, seen)[0][77] == NONE and WM.partition(mass, seen)[2] == 6


def test_properties_on_random_rows():
    rng = np.random.default_rng(7)
    for trial in range(200):
        n = int(rng.integers(1, 257))
        at = np.sort(rng.choice(256, n, replace=False))
        masses = (10.0 ** rng.uniform(-30, 3, n)).astype(F) if trial % 2 else rng.integers(0, 4, n).astype(F)
        mass, seen = row(masses, at)
        world, weights, total = WM.partition(mass, seen)
        assert ((world != NONE) == seen).all() and (world[seen] < 4).all()  # every entry in exactly one world
        if total <= 0:
            assert (world[seen] == 0).all() and np.array_equal(bits(weights), bits([0.25] * 4))
            continue
        # reach is non-increasing with the world
        for w in range(3):
            hi, lo = mass[world == w], mass[world > w][mass[world > w] == mass[world > w]]
            assert not hi.size or not lo.size or hi.min() >= lo.max()
        # the weight of a reached world is its masses folded in sorted order, over the total; an unreached one is 0
        order = sorted(at, key=lambda b: -float(mass[b]))
        for w in range(4):
            acc = F(0)
            for b in order:
                if world[b] == w:
                    acc = F(acc + mass[b])
            want = F(acc / total) if (world == w).any() else F(0)
            assert bits(weights[w]) == bits(want)
        reached = [w for w in range(4) if (world == w).any()]
        assert reached == list(range(len(reached)))  # worlds fill from 0 without a gap


def test_belief_of_the_root():
    r = Recall(0, HOLE)
    bel = WM.belief(r, {})
    status, mass, seen = RM.opponent_range(r, {})
    assert bel["status"] == status == RM.OK and bel["count"] == 1225
    assert np.array_equal(bits(bel["mass"]), bits(mass)) and np.array_equal(bel["seen"], seen)
    world, weights, _ = WM.partition(mass, seen)
    assert np.array_equal(bel["world"], world) and np.array_equal(bits(bel["weights"]), bits(weights))
    assert (bel["hole_world"][:1225] < 4).all() and (bel["hole_world"][1225:] == NONE).all()
    holes = RM.hand_iterator(HOLE)
    assert all(bel["hole_world"][j] == world[WM.hash_bucket(0, holes[j], 0)] for j in range(0, 1225, 97))
    bad = WM.belief(Recall(0, cards(3, 50), [FLOP], [ON.Open(2), ON.E_CALL, ON.E_DRAW]), {})
    assert bad["status"] == RM.CARDS and (bad["world"] == NONE).all() and (bad["hole_world"] == NONE).all()
    assert np.array_equal(bits(bad["weights"]), bits([0.25] * 4))


def test_draws_and_picks():
    deal = WM.Deal(11, WM.deal_id(5, 2, 64, 63))
    assert deal.deal_id == 7 * 64 + 63
    assert all(deal.draw(c) == FM.node_hash(11, 1, deal.deal_id, c) for c in (0, 1, 2, 77, 20001))
    assert WM.deal_id((1 << 64) - 1, 1, 3, 2) == 2  # wrapping
    free = [c for c in range(52) if not (HOLE | FLOP) >> c & 1]
    seen_pairs = set()
    for a in range(3000):
        c0, c1 = WM.attempt(deal, a, free)
        assert c0 != c1 and c0 in free and c1 in free  # always two distinct free cards
        seen_pairs.add((c0, c1))
    assert len(seen_pairs) > 1500 and any(c0 < c1 for c0, c1 in seen_pairs) and any(c0 > c1 for c0, c1 in seen_pairs)
    # the second pick skips the first card: pick k of the rest is card k below it and card k + 1 from it on
    assert WM.attempt(deal, 5, free) == WM.attempt(WM.Deal(11, deal.deal_id), 5, free)


def test_draw_world():
    w = np.array([0.5, 0.25, 0.25, 0.0], F)
    assert [WM.draw_world(w, F(u)) for u in (0.0, 0.49, 0.5, 0.74, 0.75, 0.999)] == [0, 0, 1, 1, 2, 2]
    assert WM.draw_world(w, F(1.0)) == 2  # no running sum exceeds x: the highest world of non-zero weight
    assert WM.draw_world(np.zeros(4, F), F(0.3)) == 0


def test_restrict_is_deterministic_and_consistent():
    r = Recall(0, HOLE, [FLOP], [ON.Open(2), ON.E_CALL, ON.E_DRAW, ON.E_CHECK])
    bel = WM.belief(r, {})
    assert bel["status"] == RM.OK and bel["count"] == 1081 and all((bel["hole_world"][:1081] == w).any() for w in range(4))
    worlds = np.array([0, 1, 2, 3, NONE, NONE, 9, 3], np.uint8)
    first = WM.restrict(r, bel, 3, 8, worlds, seed=5, first_id=10)
    again = WM.restrict(r, bel, 0, 8, worlds, seed=5, first_id=13)  # (seed, deal_id) decide: first_id + r is all that counts
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    other = WM.restrict(r, bel, 3, 8, worlds, seed=6, first_id=10)
    assert not np.array_equal(first[0], other[0])
    holes, out, attempts = first
    assert (holes[6], out[6], attempts[6]) == (0, NONE, 0)  # a malformed request
    assert list(out[:4]) == [0, 1, 2, 3] and out[7] == 3 and all(o < 4 for o in out[4:6])
    candidates = RM.hand_iterator(HOLE | FLOP)
    for d in (0, 1, 2, 3, 4, 5, 7):
        h = int(holes[d])
        assert RM.popcount(h) == 2 and not h & (HOLE | FLOP) and attempts[d] < WM.MAX_REJECTIONS
        assert bel["hole_world"][candidates.index(h)] == out[d]
    assert attempts.max() > 0
    # a malformed recall: nothing is dealt
    bad = WM.belief(Recall(0, HOLE, [FLOP], [25]), {})
    holes, out, attempts = WM.restrict(Recall(0, HOLE, [FLOP], [25]), bad, 0, 4)
    assert bad["status"] == RM.EDGE and not holes.any() and (out == NONE).all() and not attempts.any()


def test_abi_names_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "rp_mi355x.h")).read()
    for name in ("rp_nlhe_partition", "rp_nlhe_belief", "rp_nlhe_restrict"):
        for form in (name, name + "_device"):
            assert re.search(r"RP_API int %s\(" % form, header) and form in _lib._SIGNATURES
    for macro, value in (("RP_NLHE_WORLDS", WM.WORLDS), ("RP_NLHE_MAX_REJECTIONS", WM.MAX_REJECTIONS), ("RP_WORLD_NONE", WM.WORLD_NONE)):
        m = re.search(r"#define %s (\w+)u" % macro, header)
        assert m and int(m.group(1), 0) == value == getattr(_lib, macro)
    assert (N.WORLDS, N.MAX_REJECTIONS, N.WORLD_NONE) == (WM.WORLDS, WM.MAX_REJECTIONS, WM.WORLD_NONE)
    assert all(hasattr(N.NlheSolver, f) for f in ("partition", "belief", "restrict", "partition_device", "belief_device", "restrict_device"))

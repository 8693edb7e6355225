"""What the dense MCCFR solver must compute, restated by hand in Python.  TEST INFRASTRUCTURE ONLY.

Shared by tests/test_oracle_independent.py (built-in games) and the caller-built tables of tests/game_tables.py: the enumeration of
every externally sampled tree with the regret vector of each walker infoset in it (exact rationals), and the counter RNG's hash and
draws (include/rp_math.h) on Python integers.  Nothing here shares code with the oracle or the kernels.
"""
from __future__ import annotations

import itertools
from fractions import Fraction

import numpy as np


def sampled_trees(g, walker):
    """every externally-sampled tree of the game for `walker`: chance and opponent states keep ONE child (all
    alternatives enumerated), walker states keep all (sample/external.rs:17-64).  A tree is a dict state -> kept children."""
    t = g.table

    def expand(state):
        st = t.states[state]
        if st.n_children == 0:
            yield {}
            return
        kids = [t.children[st.offset + a] for a in range(st.n_children)]
        if st.turn == walker:
            for combo in itertools.product(*[list(expand(k)) for k in kids]):
                tree = {state: list(enumerate(kids))}
                for sub in combo:
                    tree.update(sub)
                yield tree
        else:
            for a, k in enumerate(kids):
                for sub in expand(k):
                    tree = {state: [(a, k)]}
                    tree.update(sub)
                    yield tree

    return expand(t.train_root)


def hand_decisions(g, tree, walker):
    """CfrFlow::dfs (flow.rs:64-87) for every walker infoset of one sampled tree of a fresh profile: regret
    matching is uniform and the sampling distribution is uniform, so an opponent edge carries sigma / q = 1 and a walker
    edge sigma = 1/|choices| below the root (flow.rs:182-216); chance edges carry 1."""
    t = g.table

    def value(state):  # recursed_value with relative / sampling reach folded in (exact rationals)
        st = t.states[state]
        if st.n_children == 0:
            return Fraction(t.payoffs[st.offset * t.n_players + walker]).limit_denominator(1 << 20)
        kept = tree[state]
        if st.turn == walker:
            return sum(value(k) for _, k in kept) / st.n_children
        return sum(value(k) for _, k in kept)  # one child; sigma / q = 1 (or chance: 1)

    out = []
    for state, kept in tree.items():
        st = t.states[state]
        if st.turn != walker:
            continue
        vals = [value(k) for _, k in kept]  # ancestor_reach = 1: every non-walker ancestor edge has sigma = q
        ev = sum(vals) / len(vals)
        out.append((st.info, tuple(float(v - ev) for v in vals), float(ev)))
    return out


# ---- the counter RNG (include/rp_math.h) ------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def _mix64(z):
    z ^= z >> 30
    z = (z * 0xbf58476d1ce4e5b9) & _M64
    z ^= z >> 27
    z = (z * 0x94d049bb133111eb) & _M64
    return z ^ (z >> 31)


def node_hash(seed, epoch, tree, key):  # rp_node_hash, restated on Python integers
    h = _mix64((seed + 0x9e3779b97f4a7c15) & _M64)
    h = _mix64(h ^ ((epoch * 0xd1342543de82ef95 + 0x632be59bd9b4e019) & _M64))
    h = _mix64(h ^ ((tree * 0xaf251af3b0f025b5 + 0x2545f4914f6cdd1d) & _M64))
    # the per-draw half: Murmur3's 32-bit finaliser over the low word and the folded key, the high word multiplied in
    lo, hi, k = h & 0xffffffff, h >> 32, (key ^ (key >> 32)) & 0xffffffff
    x = lo ^ k
    x ^= x >> 16
    x = (x * 0x85ebca6b) & 0xffffffff
    x ^= x >> 13
    x = (x * 0xc2b2ae35) & 0xffffffff
    x ^= x >> 16
    x = ((x ^ hi) * 0x9e3779b1) & 0xffffffff
    x ^= x >> 15
    return x << 32


def u01(h):  # rp_u01: the top 24 bits as a float in [0, 1)
    return np.float32(h >> 40) * np.float32(5.9604644775390625e-8)


def pick_uniform(h, n):  # rp_pick_uniform: the top 32 bits scaled to 0..n-1
    return ((h >> 32) * n) >> 32


def chance_draw(seed, epoch, tree, state, n):
    """the outcome the counter RNG draws at chance state `state` of tree `tree` (the draw's key is 0x80000000 | state)"""
    return pick_uniform(node_hash(seed, epoch, tree, 0x80000000 | state), n)

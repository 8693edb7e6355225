"""The packed-row skeleton traversal evaluates two round-2 sub-trees that can never be live in the same tree ONCE (the pair below an
opponent node: csrc/traverse_static.hpp, sk_exclusive_pair), and the two terminal children of an opponent node with one division.
Every live node must still see the operations it saw before, so the tables and counters are compared with the CPU oracle bit for
bit after every step — and with the child-record traversal (RP_TRAV_NO_FLAT=1), which merges nothing.

The batches: one lane; a ragged 256-tree chunk; exactly one chunk; one tree in a second chunk; several chunks.  Four steps: both
walkers twice.  The oracle's own Decisions say that the 257-tree batches hold every pattern the merge has to tell apart.
"""
import functools

import numpy as np
import pytest

import oracle
from robopoker_amd import Game
from robopoker_amd.mccfr import Solver

STEPS = 4
SEED = 101  # chosen with the CPU oracle: every pattern below occurs in the 257-tree batches of all (sampling, draw, mode) triples
BATCHES = [1, 255, 256, 257, 1357]
SAMPLINGS = ["external", "prunable", "pluribus"]
RNGS = ["counter", "reference"]


def hyper():
    hp = oracle.default_hyper()
    hp.prune_warmup, hp.prune_threshold, hp.prune_explore = 2, -0.05, 0.1  # pruning bites from the third step on
    return hp


def assert_tables_equal(a: np.ndarray, b: np.ndarray, what: str):
    for f in ("visits", "regret", "weight", "payoff"):
        if a[f].dtype.kind == "f":
            assert not np.isnan(a[f]).any(), f"{what}: NaN in {f}"
        assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), f"{what}: {f} differs bitwise"


@functools.lru_cache(maxsize=None)
def oracle_trace(game, sampling, rng, mode, batch, steps=STEPS, seed=SEED):
    """(table, counters) of the oracle after each step; computed once per case, shared by the merged and the unmerged run"""
    ora = oracle.OracleSolver(Game(game), "linear", "linear", sampling, batch=batch, seed=seed, hyper=hyper())
    if rng == "reference":
        ora.set_rng("reference")
    out = []
    for _ in range(steps):
        if mode == "composed":
            ora.step_world(1)
        else:
            ora.step()
        out.append((ora.export(), ora.counters()))
    return out


def run_against_oracle(game, sampling, rng, mode, batch, what, steps=STEPS):
    s = Solver(Game(game), "linear", "linear", sampling, batch=batch, seed=SEED, hyper=hyper())
    assert s.kernel_variant() == "static"
    if rng == "reference":
        s.set_rng("reference")
    if mode == "composed":
        s.set_update_mode("composed")
    for step, (want, counters) in enumerate(oracle_trace(game, sampling, rng, mode, batch, steps)):
        s.step()
        assert_tables_equal(s.export(), want, f"{what}, step {step}")
        assert s.counters() == counters, f"{what}, step {step}: (nodes, infos)"
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("mode", ["composed", "ordered"])
@pytest.mark.parametrize("rng", RNGS)
@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("game", ["kuhn", "leduc"])
def test_merged_traversal_equals_the_oracle(gpu, game, sampling, rng, mode, batch):
    s = run_against_oracle(game, sampling, rng, mode, batch, "packed rows (merged)")
    assert s.traversal_rows_bytes() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("mode", ["composed", "ordered"])
@pytest.mark.parametrize("rng", RNGS)
@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("game", ["kuhn", "leduc"])
def test_unmerged_child_records_give_the_same_bits(gpu, monkeypatch, game, sampling, rng, mode, batch):
    monkeypatch.setenv("RP_TRAV_NO_FLAT", "1")
    s = run_against_oracle(game, sampling, rng, mode, batch, "child records (unmerged)")
    assert s.traversal_rows_bytes() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["composed", "ordered"])
def test_leduc_wide_same_skeleton(gpu, mode):
    s = run_against_oracle("leduc_wide", "external", "counter", mode, 512, "leduc_wide", steps=2)
    assert s.traversal_rows_bytes() > 0


# ---- what the 257-tree batches contain, by the oracle's own Decisions ------------------------------------------------------------
# Leduc infoset names: "rank|history" in round 1, "rank|board|history" in round 2; the history of a round-2 infoset starts with the
# round-1 line that led there: "XX" (sub-tree A, check-check), "XRC" (B, check-raise-call), "RC" (C, raise-call).
LINES = {"A": "XX", "B": "XRC", "C": "RC"}
# what player 0 has won when player 1 folds to its round-2 raise: the opponent's ante, and its round-1 bet (2) where there was one
FOLD_WIN = {"A": 1.0, "B": 3.0, "C": 3.0}


def tree_patterns(g, decisions, walker, default_tables):
    """per tree: the round-2 sub-trees that hold a walker Decisions, and whether the Decisions PROVE that the opponent folded to the
    walker's round-2 raise.  With u_e = regret[e] + payoff the value of edge e (up to rounding):
    walker 0, OPEN', tables at their defaults (the first step): every importance weight is 1, so the raise is worth exactly the
      terminal's payoff — FOLD_WIN after a fold, +-(FOLD_WIN + 4) or a split 0 after a call;
    walker 1, CHECKED': the check ends in the showdown, the raise in the opponent's fold (the walker wins) or call (the SAME showdown,
      for more): a walker that loses the showdown (u_0 < 0) and wins with the raise (u_1 > 0) has seen a fold, whatever the weights."""
    names = [g.info_name(i) for i in range(g.n_infos)]
    trees = {}
    for d in decisions:
        t = trees.setdefault(d["tree"], {"sub": set(), "fold": False})
        parts = names[d["info"]].split("|")
        if len(parts) != 3:
            continue
        for sub, line in LINES.items():
            # "RC.." is C's alone: B's line starts with X
            if not (parts[2].startswith(line) and parts[2][len(line):] in ("", "X", "R", "XR")):
                continue
            t["sub"].add(sub)
            if d["expanded"] != 3:
                continue
            u0, u1 = d["regret"][0] + d["payoff"], d["regret"][1] + d["payoff"]
            if walker == 0 and default_tables and parts[2] == line:
                t["fold"] = t["fold"] or abs(u1 - FOLD_WIN[sub]) < 0.25
            if walker == 1 and parts[2] == line + "X":
                t["fold"] = t["fold"] or (u0 < -1e-3 and u1 > 1e-3)
    return trees


@pytest.mark.parametrize("mode", ["composed", "ordered"])  # the tables, and with them the later steps' trees, differ between the two
@pytest.mark.parametrize("rng", RNGS)
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_the_257_tree_batches_hold_every_pattern(sampling, rng, mode):
    g = Game("leduc")
    ora = oracle.OracleSolver(g, "linear", "linear", sampling, batch=257, seed=SEED, hyper=hyper())
    if rng == "reference":
        ora.set_rng("reference")
    seen = {0: set(), 1: set()}
    for step in range(STEPS):
        walker = step % 2
        for t in tree_patterns(g, ora.batch(), walker, step == 0).values():
            seen[walker] |= {f"{s} live" for s in t["sub"]}
            seen[walker] |= {f"{s} dead" for s in "ABC" if s not in t["sub"]}
            if t["fold"]:
                seen[walker].add("fold to a round-2 raise")
            # the pairs the traversal merges are exclusive in every tree
            if walker == 0:
                assert not {"A", "B"} <= t["sub"], "walker 0: CHECKED is the opponent's node, one of A / B"
            else:
                assert not ("C" in t["sub"] and t["sub"] & {"A", "B"}), "walker 1: OPEN is the opponent's node, C or A / B"
        if mode == "composed":
            ora.step_world(1)
        else:
            ora.step()
    want = {"A live", "B live", "C live", "C dead", "A dead", "B dead", "fold to a round-2 raise"}
    assert want <= seen[0], f"walker 0 misses {want - seen[0]}"
    assert want <= seen[1], f"walker 1 misses {want - seen[1]}"

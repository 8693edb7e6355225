"""Pins the model the match kernel is compared against (tests/nlhe_match_model.py) without a GPU: every recorded hand replays legally
through the oracle and settles to its `won`, the hero flip, the mirrored pairs, the fish, Dirac's tie, the sampling order, the
statistics (host-only arithmetic of the library), the ABI — and, on the model's trace of the GPU test's batches
(tests/nlhe_match_cases.py), every case the kernel has to get right, so that a changed seed cannot silently empty the GPU test."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nlhe_aivat_model as AM
import nlhe_match_cases as K
import nlhe_match_model as MM
import oracle_nlhe as ON
from robopoker_amd import _lib
from robopoker_amd.nlhe import AIVAT_DTYPE, NlheSolver

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def by_hand(trace):
    out = {}
    for ev in trace:
        out.setdefault(ev["hand"], []).append(ev)
    return out


def last_kind(w):
    return w["plays"][-1][0] if w["plays"] else None


def longest_street(w):
    """the most plays any one street of the hand saw, counted by replaying it"""
    stacks = w["stacks"] if w["stacks"] != (0, 0) else (ON.STACK, ON.STACK)
    g, count = AM._start(w["dealer"], stacks, w["holes"]), {}
    for k, c in w["plays"]:
        while AM._turn(g) == ON.CHANCE:
            g = AM._consume(g, ON.Draw(w["draws"][AM._street(g)]))
        count[AM._street(g)] = count.get(AM._street(g), 0) + 1
        g = AM._consume(g, (k, c, 0))
    return max(count.values())


def test_every_recorded_hand_replays_legally_and_settles_to_won():
    m = K.model()
    for name in K.NAMES:
        args = K.CONFIGS[K.NAMES.index(name)][2]
        for w in m.want[name]:
            assert w["status"] == MM.OK, name
            stacks = w["stacks"] if w["stacks"] != (0, 0) else (ON.STACK, ON.STACK)
            g = AM._start(w["dealer"], stacks, w["holes"])
            for k, c in w["plays"]:
                while AM._turn(g) == ON.CHANCE:
                    assert w["draws"][AM._street(g)] != 0
                    g = AM._consume(g, ON.Draw(w["draws"][AM._street(g)]))
                assert AM._turn(g) >= 0 and AM._allowed(g, (k, c, 0)), (name, w)
                g = AM._consume(g, (k, c, 0))
            while AM._turn(g) == ON.CHANCE:  # the run-out of an all-in
                g = AM._consume(g, ON.Draw(w["draws"][AM._street(g)]))
            assert AM._turn(g) == ON.TERMINAL and all(d == 0 for d in w["draws"][AM._street(g):]), (name, w)
            assert ON.Game(g, None).settlements()[args.hero][1] == w["won"] and w["seat"] == args.hero, (name, w)


def test_hero_flipped_negates_won_and_changes_nothing_else():
    m = K.model()
    for a, b in zip(m.want["main"], m.want["main hero 1"]):
        assert a["won"] == -b["won"] and (a["seat"], b["seat"]) == (0, 1)
        assert {k: v for k, v in a.items() if k not in ("won", "seat")} == {k: v for k, v in b.items() if k not in ("won", "seat")}
    assert any(w["won"] != 0 for w in m.want["main"])


def test_mirrored_pairs_carry_one_board_and_swapped_holes():
    m = K.model()
    first = K.CONFIGS[K.NAMES.index("main")][2].first_id
    hands = {first + i: w for i, w in enumerate(m.want["main"])}
    pairs = [(hands[i], hands[i + 1]) for i in hands if i % 2 == 0 and i + 1 in hands]
    assert first % 2 == 1 and len(pairs) == 32
    for a, b in pairs:
        assert a["holes"] == b["holes"][::-1] and a["holes"][0] != a["holes"][1]
        reached = min(sum(d != 0 for d in a["draws"]), sum(d != 0 for d in b["draws"]))
        assert a["draws"][:reached] == b["draws"][:reached]
        full = MM.deal(K.SEED, (first + m.want["main"].index(a)) >> 1)
        assert a["holes"] == full[:2] and list(a["draws"][:reached]) == full[2][:reached]
    assert any(sum(d != 0 for d in a["draws"]) == 3 for a, _ in pairs)


def test_the_fish_never_shoves_and_reads_no_table():
    m = K.model()
    seen = 0
    for name in K.NAMES:
        for ev in m.trace[name]:
            if ev["agent"] == MM.FISH:
                seen += 1
                assert ev["asked"][0] != ON.SHOVE and "key" not in ev and not ev["rejected"], name
    assert seen > 100


def test_dirac_returns_the_last_of_equal_maxima_in_edge_order():
    # a row built for it: Raise(1/3) = code 11 and Raise(1/1) = code 15 share the maximum; in slot order 11 comes first, in Edge's
    # order Raise(Odds(1, 1)) < Raise(Odds(1, 3)): the LAST maximal edge is 11
    policy = {MM.edge_key(e): (e, F(p)) for e, p in ((11, 0.4), (12, 0.1), (15, 0.4), (ON.E_FOLD, 0.1))}
    assert [e for _, (e, _) in sorted(policy.items())] == [ON.E_FOLD, 15, 12, 11] and MM.argmax(policy) == 11
    # Shove is last of all, Fold first, the opens ascend by chips, and an Open sorts before every Raise
    order = sorted(range(1, 20), key=MM.edge_key)
    assert order == [1, 2, 3, 4, 6, 7, 8, 9, 15, 12, 11, 10, 18, 13, 19, 17, 14, 16, 5]
    # in the batches: a dirac decision with tied maxima whose first and last differ
    m = K.model()
    ties = 0
    for name in K.NAMES:
        for ev in m.trace[name]:
            if ev["agent"] == MM.DIRAC:
                w = m.rows[ev["seat"]].get(ev["key"])
                dist = MM.PM.distribution("averaged", np.zeros(9, F) if w is None else w, len(ev["slots"]))
                top = [e for e, p in zip(ev["slots"], dist) if p == dist[: len(ev["slots"])].max()]
                if len(top) > 1:
                    ties += 1
                    assert ev["edge"] == max(top, key=MM.edge_key), (name, ev)
    assert ties > 10


def test_the_header_states_the_rank_of_every_edge_code():
    header = open(os.path.join(ROOT, "include", "rp_mi355x.h")).read()
    ranks = [int(x) for x in re.search(r"#define RP_EDGE_ORD_RANKS \{([^}]*)\}", header).group(1).split(",")]
    order = sorted(range(1, 20), key=MM.edge_key)
    assert ranks[0] == 31 and [ranks[e] for e in order] == list(range(19))


def conditions(m):
    """the cases the kernel has to get right, each as (description, does it occur in the batches)"""
    main, snap, trace = m.want["main"], m.want["main snap"], by_hand(m.trace["main"])
    first = K.CONFIGS[K.NAMES.index("main")][2].first_id
    streets = [max(e["street"] for e in trace[first + i]) for i in range(len(main))]
    sampled = [e for name in K.NAMES for e in m.trace[name] if e["agent"] == MM.BLUEPRINT]
    raises = lambda e: [x for x in e["slots"] if x >= 10]  # noqa: E731
    return [
        ("a preflop fold", any(w["draws"] == (0, 0, 0) and last_kind(w) == ON.FOLD for w in main)),
        ("a showdown on the river", any(w["draws"][2] and last_kind(w) != ON.FOLD and s == 3 for w, s in zip(main, streets))),
        ("an all-in and a call before the river: streets dealt, no plays on them",
         any(w["draws"][2] and last_kind(w) != ON.FOLD and s < 2 for w, s in zip(main, streets))),
        ("a hand with rejected > 0 under snap = 0 whose twin under snap = 1 differs",
         any(a["rejected"] > 0 and K.pack([a]).tobytes() != K.pack([b]).tobytes() for a, b in zip(main, snap))),
        ("a decision on an absent row", any(not e["found"] for e in m.trace["main"])),
        ("a hand past 12 edges on one street", longest_street(m.want["long street"][1]) > 12),
        ("a decision after the hand's 12th edge", any(e["n_before"] >= 12 for e in sampled)),
        ("dealer = 2 gives both dealers", {w["dealer"] for w in main} == {0, 1} and all(w["dealer"] == (first + i) & 1 for i, w in enumerate(main))),
        ("a sampled decision that sampling in slot order would decide otherwise", any(e["by_slot_order"] != e["edge"] for e in sampled)),
        ("a sampled decision over raises whose slot order and Ord order differ, and one over an Open beside a Raise-free grid",
         any(raises(e) != sorted(raises(e), key=MM.edge_key) for e in sampled) and any(6 in e["slots"] for e in sampled)),
        ("the second table decides some hands otherwise", 0 < sum(a != b for a, b in zip(main, m.want["main one table"])) < len(main)),
        ("a rejected play of a blueprint agent and one of a dirac agent",
         all(any(e["rejected"] and e["agent"] == kind for n in K.NAMES for e in m.trace[n]) for kind in (MM.BLUEPRINT, MM.DIRAC))),
        ("both tables fit", all(t[0].size <= K.SLOTS - 64 for t in m.tables)),
    ]


def test_every_case_occurs_in_the_batches():
    missing = [what for what, ok in conditions(K.model()) if not ok]
    assert not missing, missing


def test_a_hand_does_not_depend_on_the_batch_around_it():
    m = K.model()
    args = K.CONFIGS[K.NAMES.index("main")][2]
    alone = MM.Args(**dict(args.kwargs(), first_id=args.first_id + 40))
    assert MM.match(3, alone, m.rows) == m.want["main"][40:43]


def test_summarize():
    rng = np.random.default_rng(7)
    series = [rng.integers(-400, 400, 1000), rng.integers(-3, 3, 17), np.full(5, 7), np.zeros(3), np.array([4]), np.zeros(0),
              np.array([32767, -32768])]
    for x in series:
        got, want = NlheSolver.match_summary(x.astype(np.int16)), MM.summarize(x.astype(np.int16))
        assert got["hands"] == want["hands"] == x.size
        for k in ("total_bb", "bb_per_100", "stddev", "confidence"):
            assert np.float64(got[k]).view(np.uint64) == np.float64(want[k]).view(np.uint64), (k, got[k], want[k])
    one = NlheSolver.match_summary(np.array([4], np.int16))
    assert one == dict(hands=1, total_bb=2.0, bb_per_100=200.0, stddev=0.0, confidence=0.0)
    assert NlheSolver.match_summary(np.zeros(0, np.int16)) == dict(hands=0, total_bb=0.0, bb_per_100=0.0, stddev=0.0, confidence=0.0)
    with pytest.raises(_lib.RpError):
        _lib.check(_lib.load().rp_match_summarize(1, None, C.byref(_lib.MatchSummary())))


def test_abi():
    assert C.sizeof(_lib.NlheMatchArgs) == 32 and C.sizeof(_lib.MatchSummary) == 40 and AIVAT_DTYPE.itemsize == 192
    header = open(os.path.join(ROOT, "include", "rp_mi355x.h")).read()
    for n in ("rp_nlhe_match", "rp_nlhe_match_device", "rp_match_summarize"):
        assert re.search(r"RP_API\s+int\s+" + n + r"\s*\(", header) and n in _lib.declared_symbols() and hasattr(_lib.load(), n)
    assert re.search(r"RP_API\s+void\s+rp_nlhe_match_args_default\s*\(", header) and "rp_nlhe_match_args_default" in _lib.declared_symbols()
    assert all("RP_AGENT_%s = %d" % (k.upper(), v) in header for k, v in _lib.AGENT.items()) and _lib.AGENT == MM.AGENT
    a = _lib.NlheMatchArgs()
    _lib.load().rp_nlhe_match_args_default(C.byref(a))
    assert (a.seed, a.first_id, tuple(a.stacks), tuple(a.agent), a.dealer, a.hero, a.mirror, a.snap, a.board_mode, bytes(a.reserved)) == \
        (0, 0, (0, 0), (0, 0), 2, 0, 0, 0, 1, bytes(5))

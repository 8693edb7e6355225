"""Pins the model the AIVAT kernel is compared against (tests/nlhe_aivat_model.py) without a GPU: correction.rs's own unit-test
properties on seeded inputs, one hand worked by hand, the sign rules, rp_aivat_summarize (host-only arithmetic of the library), and —
on the model's trace of the GPU test's batch (tests/nlhe_aivat_cases.py) — every case the kernel has to get right, so that a batch
that no longer exercises one of them fails here before anything runs on a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nlhe_aivat_cases as K
import nlhe_aivat_model as AM
import nlhe_policy_model as PM
import oracle_nlhe as ON
from robopoker_amd import _lib
from robopoker_amd.nlhe import AIVAT_DTYPE, AivatHand, NlheSolver

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def random_policy(rng):
    n = int(rng.integers(2, 6))
    return [(F(rng.uniform(0.01, 10.0)), F(rng.uniform(-100.0, 100.0))) for _ in range(n)]


# ---- the eight properties of arena/src/correction.rs's unit tests
def test_uniform_ev_yields_zero_correction_for_any_action():
    rng = np.random.default_rng(1)
    for _ in range(100):
        ev, n = F(rng.uniform(-100, 100)), int(rng.integers(2, 6))
        policy = [(F(rng.uniform(0.01, 10.0)), ev) for _ in range(n)]
        assert all(abs(AM.action_correction(policy, i)) < 1e-4 for i in range(n))


def test_correction_sums_to_zero_under_policy():
    rng = np.random.default_rng(2)
    for _ in range(100):
        policy = random_policy(rng)
        total = AM.fold32(w for w, _ in policy)
        assert abs(AM.fold32(F(F(w / total) * AM.action_correction(policy, i)) for i, (w, _) in enumerate(policy))) < 1e-3


def test_best_action_negative_worst_action_positive():
    rng = np.random.default_rng(3)
    for _ in range(100):
        policy = random_policy(rng)
        v = [float(x) for _, x in policy]
        assert AM.action_correction(policy, v.index(max(v))) <= 1e-6
        assert AM.action_correction(policy, v.index(min(v))) >= -1e-6


def test_missing_idx_yields_zero_correction():
    rng = np.random.default_rng(4)
    for _ in range(100):
        policy = random_policy(rng)
        assert AM.action_correction(policy, None) == 0.0 and AM.action_correction(policy, 999) == 0.0


def test_chance_correction_is_antisymmetric_and_zero_when_equal():
    rng = np.random.default_rng(5)
    for _ in range(100):
        a, b = F(rng.uniform(-100, 100)), F(rng.uniform(-100, 100))
        assert abs(AM.chance_correction(a, b) + AM.chance_correction(b, a)) < 1e-6
        assert AM.chance_correction(a, a) == 0.0


def test_empty_and_zero_weight_policies_yield_zero():
    assert AM.strategy_ev([]) == 0.0 and AM.action_correction([], 0) == 0.0 and AM.action_correction([], None) == 0.0
    rng = np.random.default_rng(6)
    for _ in range(100):
        assert AM.strategy_ev([(F(0.0), F(rng.uniform(-100, 100))) for _ in range(int(rng.integers(2, 6)))]) == 0.0


# ---- one hand worked by hand
def test_a_hand_worked_by_hand():
    """Seat 0 deals, posts 1 and folds to the big blind.  One node: seat 0 to act before the flop, no edge behind it (past = 0),
    aggression 0, so the choices are Open(2) Open(3) Open(4) Open(5) Shove Call Fold = edges 6 7 8 9 5 4 2, and Fold is slot 6.
    With weights 1 1 0 0 0 2 4 (total 8) and payoffs 8 -8 100 100 100 2 -1 the strategy's value is
    1/8 * 8 + 1/8 * -8 + 0 + 0 + 0 + 2/8 * 2 + 4/8 * -1 = 1 - 1 + 0.5 - 0.5 = 0, the observed value is -1: the correction is +1.
    For hero = seat 0 it is added to hero; for hero = seat 1 it is subtracted from villain.  No chance node: chance = 0."""
    holes = K.HOLES
    rec = AM.Recorder()
    AM.corrections(AivatHand(holes, (), [("fold", 0)]), rec)
    key, = rec.asked
    assert key[1] >> 8 == 0 and key[0] == 0 and list(PM.edges(key[2])[: PM.nch(key[2])]) == [6, 7, 8, 9, 5, 4, 2]
    w = np.array([1, 1, 0, 0, 0, 2, 4, 9, 9], F)
    v = np.array([8, -8, 100, 100, 100, 2, -1, 9, 9], F)
    got = AM.corrections(AivatHand(holes, (), [("fold", 0)], seat=0), {key: (w, v)})
    assert got == (AM.OK, F(1.0), F(0.0), F(0.0), F(1.0), 1, 0)
    got = AM.corrections(AivatHand(holes, (), [("fold", 0)], seat=1), {key: (w, v)})
    assert got == (AM.OK, F(0.0), F(-1.0), F(0.0), F(-1.0), 1, 0)


# ---- the batch
def conditions(m):
    """the cases the kernel has to get right, each as (description, does it occur in the batch)"""
    past, present, choices, _ = m.table
    slot, home = K.placement(past, present, choices)
    off_home = {(int(p), int(q), int(c)) for p, q, c, s, h in zip(past, present, choices, slot, home) if s != h}
    act, cha = m.nodes("action"), m.nodes("chance")
    ref = {n: m.trace[K.NAMES.index(n)] for n in ("streets seat 0", "streets at the node")}
    pairs = [(a, b) for a, b in zip(ref["streets seat 0"], ref["streets at the node"]) if a["kind"] == "action"]
    seat0, seat1 = m.of("streets seat 0"), m.of("streets seat 1")
    return [
        ("an action node with a row and the edge among its slots", any(e["value"] is not None and e["idx"] is not None for e in act)),
        ("an action node with no row", any(not e["found"] for e in act)),
        ("a row of zero total weight", any(e["zero"] for e in act)),
        ("a probe that ends off its home slot, at an action node and at a chance node",
         any(e["found"] and e["key"] in off_home for e in act) and any(k in off_home for e in cha for k, found in e["keys"] if found)),
        ("a snapped raise that is not the nearest grid edge below", any(e["below"] is not None and e["below"] != e["edge"] for e in act)),
        ("a raise between two grid edges, the first taken", m.trace[K.NAMES.index("streets seat 0")][0]["edge"] == ON.Open(2)),
        ("a raise where the grid is empty", any(e["below"] is None and e["edge"] == ON.E_SHOVE and e["street"] == 1
                                                 for e in m.nodes("action", ["off grid"]))),
        ("a chance node with a dropped deal and a NULL baseline among the joined", any(e["dropped"] and e["null"] for e in cha)),
        ("a chance node that is None because the observed bucket has no row",
         any(e["sign"] and not e["obs_row"] and e["dropped"] < 44 for e in cha)),
        ("a chance node with a value under each sign", {e["sign"] for e in cha if e["value"] is not None} == {1, -1}),
        ("a board_mode 0 node that finds nothing where board_mode 1 finds a row", any(not a["found"] and b["found"] for a, b in pairs)),
        ("the absent hand asks and finds nothing", bool(m.trace[0]) and not any(e.get("found") or e.get("obs_row") for e in m.trace[0])),
        ("every part of the two-seat pair is non-zero", all(float(x) != 0.0 for x in seat0[1:5] + seat1[1:5])),
        ("every status is the stated one", all(w[0] == K.STATUS.get(n, AM.OK) for n, w in zip(K.NAMES, m.want))),
        ("the table fits, and about half of the infosets asked for have a row",
         past.size < K.SLOTS - 64 and 0.4 < past.size / len([k for k, r in m.rows.loaded.items()]) < 0.6),
    ]


def test_every_case_occurs_in_the_batch():
    missing = [what for what, ok in conditions(K.model()) if not ok]
    assert not missing, missing


def test_signs_and_refusals():
    m = K.model()
    a, b = m.of("streets seat 0"), m.of("streets seat 1")
    # hero <-> -villain, chance <-> -chance, total <-> -total, bit for bit
    flip = lambda x: bits(x) ^ np.uint32(0x80000000)  # noqa: E731
    assert bits(b[1]) == flip(a[2]) and bits(b[2]) == flip(a[1]) and bits(b[3]) == flip(a[3]) and bits(b[4]) == flip(a[4])
    assert a[5:] == b[5:]
    for name, w in zip(K.NAMES, m.want):
        if w[0] != AM.OK:
            assert w[1:] == (F(0.0),) * 4 + (0, 0), name
    # the plays after the fold are ignored; the all-in has two action nodes and no chance node although the board runs out
    assert m.of("after a fold")[0] == AM.OK and len(m.trace[K.NAMES.index("after a fold")]) == 2
    assert [e["kind"] for e in m.trace[K.NAMES.index("all in")]] == ["action", "action"]
    # the 12-edge cut: the river re-raise of the long hand enters `past` as the depth-0 edge 1/2, not the depth-1 edge 1/1 it is observed as
    last = m.trace[K.NAMES.index("long")][-1]
    assert ON.path_unpack(last["key"][0])[-1] == ON.RaiseOdds(1, 2) and m.trace[K.NAMES.index("long")][-2]["edge"] == ON.RaiseOdds(1, 1)


def test_pack_and_abi():
    assert AIVAT_DTYPE.itemsize == C.sizeof(_lib.AivatHand) == 192
    rec = AivatHand.pack([h for _, h in K.CASES])
    i = K.NAMES.index("stacks")
    assert tuple(rec[i]["stacks"]) == (150, 90) and rec[i]["dealer"] == 1 and rec[i]["seat"] == 1 and rec[i]["n_plays"] == 7
    assert list(rec[i]["kind"][:7]) == [4, 2, 3, 3, 3, 4, 1] and list(rec[i]["chips"][:2]) == [4, 3]
    header = open(os.path.join(ROOT, "include", "rp_mi355x.h")).read()
    for n in ("rp_nlhe_aivat", "rp_nlhe_aivat_device", "rp_aivat_summarize"):
        assert re.search(r"RP_API\s+int\s+" + n + r"\s*\(", header) and n in _lib.declared_symbols() and hasattr(_lib.load(), n)
    assert "RP_AIVAT_WITNESS = %d" % AM.WITNESS in header and _lib.RP_AIVAT_WITNESS == AM.WITNESS


def test_summarize():
    rng = np.random.default_rng(7)
    series = [rng.normal(0.3, 5.0, 1000), rng.normal(-2.0, 0.01, 17), np.full(5, 2.5), np.zeros(3), np.array([4.0]), np.zeros(0)]
    for x in series:
        x = x.astype(F)
        got, want = NlheSolver.aivat_summarize(x, 6.5), AM.summarize(x, 6.5)
        assert {k: int(bits(v).ravel()[0]) for k, v in got.items()} == {k: int(bits(v).ravel()[0]) for k, v in want.items()}, x[:4]
    flat = NlheSolver.aivat_summarize(np.full(5, 2.5, F), 6.5)
    assert flat["stderr"] == 0 and flat["reduction"] == 1 and flat["pvalue"] == 1 and flat["mean"] == F(2.5)
    with pytest.raises(_lib.RpError):
        _lib.check(_lib.load().rp_aivat_summarize(1, None, 1.0, C.byref(_lib.AivatSummary())))

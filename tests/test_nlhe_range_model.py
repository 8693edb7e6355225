"""Pins tests/nlhe_range_model.py, the naive model the GPU range tests (tests/test_gpu_nlhe_range.py) compare against, and the new
symbols of the C ABI (rp_nlhe_reaches, rp_nlhe_opponent_range and their _device forms).  No GPU."""
import ctypes as C
import os
import re

import numpy as np

import nlhe_policy_model as PM
import nlhe_range_model as RM
import oracle_nlhe as ON
from robopoker_amd import _lib
from robopoker_amd.nlhe import RECALL_DTYPE, Recall

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPEN2, RAISE_POT = ON.Open(2), ON.RaiseOdds(1, 1)


def cards(*cs):
    return sum(1 << c for c in cs)


HOLE, FLOP, TURN, RIVER = cards(51, 50), cards(3, 17, 30), cards(44), cards(9)


class SameForEveryBucket:
    """rows whose weights depend on (past, choices) only"""

    def __init__(self, by_public):
        self.by_public = by_public

    def get(self, key):
        return self.by_public.get((key[0], key[2]))


def test_root_recall_is_all_ones():
    r = Recall(0, HOLE)
    for kind, count in (("opponent", 1225), ("signalled", 1326)):
        status, holes, reach = RM.reaches(r, kind, {})
        assert status == RM.OK and holes.size == reach.size == count
        assert np.array_equal(reach.view(np.uint32), np.ones(count, F).view(np.uint32))  # the empty product
        _, _, normed = RM.reaches(r, kind, {}, normalize=True)
        assert np.array_equal(normed.view(np.uint32), (np.ones(count, F) / F(count)).view(np.uint32))  # 1225 and 1326 are exact in f32 sums


def test_enumeration_is_ascending_and_disjoint():
    r = Recall(1, HOLE, [FLOP], [OPEN2, ON.E_CALL, ON.E_DRAW])
    for kind, taken in (("opponent", HOLE | FLOP), ("signalled", FLOP)):
        _, holes, _ = RM.reaches(r, kind, {})
        h = [int(x) for x in holes]
        assert h == sorted(h) and len(set(h)) == len(h)
        assert all(RM.popcount(x) == 2 and not x & taken for x in h)
        free = 52 - RM.popcount(taken)
        assert len(h) == free * (free - 1) // 2
    # HandIterator's order is the numeric one: by high card, then low card
    assert RM.hand_iterator(0)[:4] == [0b11, 0b101, 0b110, 0b1001]


def test_two_node_history_worked_by_hand():
    # seat 0 (the button, small blind) opens to 2 bb, seat 1 raises the pot, seat 0 calls: seat 0 acted twice
    r = Recall(0, HOLE, [], [OPEN2, RAISE_POT, ON.E_CALL])
    root = ON.path_pack([6, 7, 8, 9, ON.E_SHOVE, ON.E_CALL, ON.E_FOLD])      # four opens, shove, call, fold
    facing = ON.path_pack([RAISE_POT, ON.E_SHOVE, ON.E_CALL, ON.E_FOLD])     # third raise of the street: the grid's last row
    w_root = np.array([3, 1, 1, 1, 1, 1, 0, 9, 9], F)   # slot 6 (fold) is raised to epsilon; 9s lie beyond the 7 actions
    w_facing = np.array([1, 2, 4, 1, 9, 9, 9, 9, 9], F)
    rows = SameForEveryBucket({(0, root): w_root, (ON.path_pack([OPEN2, RAISE_POT]), facing): w_facing})
    used = []
    status, holes, reach = RM.reaches(r, "signalled", rows, used=used)
    assert status == RM.OK and holes.size == 1326
    assert {(k[0], k[2]) for k, _, _ in used} == set(rows.by_public) and all(found and live for _, found, live in used)
    total = F(0)
    for x in (3, 1, 1, 1, 1, 1, PM.EPSILON):
        total = F(total + F(x))
    want = F(F(F(1.0) * F(F(3) / total)) * F(F(4) / F(8)))
    assert np.array_equal(reach.view(np.uint32), np.full(1326, want, F).view(np.uint32))
    # the opponent saw seat 1 act once; its infoset has no row: uniform over {pot raise, 2x pot raise, shove, call, fold}
    status, holes, reach = RM.reaches(r, "opponent", rows)
    five = F(0)
    for _ in range(5):
        five = F(five + PM.EPSILON)
    assert holes.size == 1225 and np.array_equal(reach.view(np.uint32), np.full(1225, F(PM.EPSILON / five), F).view(np.uint32))
    # an edge that is not among the choices: factor 0
    used = []
    _, _, reach = RM.reaches(Recall(0, HOLE, [], [ON.E_CHECK]), "signalled", rows, used=used)
    assert not reach.any() and not any(live for _, _, live in used)


def test_path_keeps_its_first_twelve_edges():
    edges = [OPEN2, RAISE_POT, ON.E_CALL, 1, 3, 3, 1, 3, 3, 1, 3, RAISE_POT, RAISE_POT, RAISE_POT, ON.E_CALL]
    r = Recall(0, HOLE, [FLOP, TURN, RIVER], edges)
    draws = RM.validate(r)
    cand = cards(0, 1)
    for subject, at in ((0, 13), (1, 14)):  # who acts at edges 13 and 14, the first nodes with more than 12 edges behind them
        nodes, _ = RM.replay(r, [HOLE, cand] if subject == 1 else [cand, HOLE], subject, draws)
        key, edge = nodes[-1]
        assert edge == edges[at]
        # the key is the one built from edges[0:12] ...
        assert ON.path_unpack(key[0]) == [ON.E_CHECK, RAISE_POT]
        # ... not from the edges really played on the river before this node
        assert edges[10:at] != [ON.E_CHECK, RAISE_POT]
        assert ON.lib().ora_path_aggression(key[0]) == 1 and RAISE_POT in PM.edges(key[2])  # depth 1: the pot raise is still offered


def test_malformed_recalls_have_a_status():
    ok = dict(pov=0, hole=HOLE, draws=[FLOP], edges=[OPEN2, ON.E_CALL, ON.E_DRAW])
    bad = {RM.EDGE: dict(edges=[OPEN2, 25]), RM.EDGE + 100: dict(edges=[0]), RM.LENGTH: dict(edges=[ON.E_CHECK] * 49),
           RM.CARDS: dict(hole=cards(3, 50)), RM.CARDS + 100: dict(hole=cards(1, 2, 4)), RM.CARDS + 200: dict(draws=[cards(1, 2)]),
           RM.CARDS + 300: dict(draws=[0, TURN]), RM.DRAW: dict(draws=[]), RM.DRAW + 100: dict(edges=[OPEN2, ON.E_CALL, ON.E_CHECK], draws=[]),
           RM.SEAT: dict(pov=2), RM.SEAT + 100: dict(stacks=(0, 5))}
    for status, change in bad.items():
        got = RM.reaches(Recall(**{**ok, **change}), "opponent", {})
        assert got[0] == status % 100 and got[1].size == 0, change
    assert RM.reaches(Recall(**ok), "opponent", {})[0] == RM.OK


def test_header_binding_and_library_agree_on_the_range_symbols():
    names = ["rp_nlhe_reaches", "rp_nlhe_reaches_device", "rp_nlhe_opponent_range", "rp_nlhe_opponent_range_device"]
    header = open(os.path.join(ROOT, "include", "rp_mi355x.h")).read()
    lib = _lib.load()
    for n in names:
        assert re.search(r"RP_API\s+int\s+" + n + r"\s*\(", header) and n in _lib.declared_symbols() and hasattr(lib, n)
    assert re.search(r"#define\s+RP_NLHE_MAX_HISTORY\s+48u", header) and re.search(r"#define\s+RP_NLHE_MAX_HOLES\s+1326u", header)
    assert (_lib.RP_NLHE_MAX_HISTORY, _lib.RP_NLHE_MAX_HOLES) == (48, 1326) and _lib.REACH == {"opponent": 0, "signalled": 1}
    for i, name in enumerate(["OK", "EDGE", "ILLEGAL", "LENGTH", "CARDS", "DRAW", "SEAT", "LOOKUP"]):
        assert re.search(r"RP_RECALL_%s = %d\b" % (name, i), header) and getattr(RM, name) == i
    assert C.sizeof(_lib.NlheRecall) == RECALL_DTYPE.itemsize == 88
    for f in ("hole", "draws", "stacks", "pov", "dealer", "n_edges", "reserved", "edges"):
        assert getattr(_lib.NlheRecall, f).offset == RECALL_DTYPE.fields[f][1], f
    packed = Recall.pack([Recall(1, HOLE, [FLOP, TURN], [6, 4, 1], stacks=(150, 90), dealer=1)])[0]
    assert (packed["hole"], list(packed["draws"]), list(packed["stacks"])) == (HOLE, [FLOP, TURN, 0], [150, 90])
    assert (packed["pov"], packed["dealer"], packed["n_edges"], list(packed["edges"][:4])) == (1, 1, 3, [6, 4, 1, 0])
    # the queries refuse a missing handle and answer an empty batch without one launch, GPU or not
    assert lib.rp_nlhe_reaches(None, 0, 0, 0, None, None, None, None, None) == _lib.RP_ERR_INVALID
    assert lib.rp_nlhe_opponent_range_device(None, 0, None, None, None, None) == _lib.RP_ERR_INVALID

"""The safe subgame re-solve from the device-resident blueprint: rp_nlhe_subgame_solve, host and _device forms, against the naive model of
tests/nlhe_subgame_model.py (pinned by tests/test_nlhe_subgame_model.py).  Results, every exported row and every traced deal are
compared as integers and bit patterns: there is no tolerance.

One batch mixes every kind of entry and belief with malformed ones between valid ones; the model is run once per module (rollouts 2
with the harvest taken after 1, 2 and 8 iterations, rollouts 1 after 1 and 2) over one blueprint decided key by key as the model asks,
which is then loaded into the table.  The beliefs of the batch are data; the chained test takes them from rp_nlhe_belief_device."""
import ctypes as C

import numpy as np
import pytest
import torch

import nlhe_depth_model as DM
import nlhe_rollout_model as FM
import nlhe_subgame_model as SM
import oracle_nlhe as ON
from nlhe_solve_common import Table, bits, cards
from robopoker_amd import _lib
from robopoker_amd.nlhe import MAX_HOLES, ORIGIN_NONE, SUBGAME_DEAL_DTYPE, SUBGAME_RESULT_DTYPE, SUBGAME_ROW_DTYPE, Frontier, NlheSolver

pytestmark = pytest.mark.gpu

OPEN2, POT = ON.Open(2), ON.RaiseOdds(1, 1)
DRAW, FOLD, CHECK, CALL = ON.E_DRAW, ON.E_FOLD, ON.E_CHECK, ON.E_CALL
BIAS, PRIOR, SEED, FIRST_ID, EPOCH, ROWS_CAP, DEALS_CAP = 5.0, 64.0, 0x5EED, 1000, 3, 176, 8
F = np.float32
NAN = float("nan")
HOLES, FLOP, TURN, RIVER = (cards(51, 50), cards(12, 25)), cards(3, 17, 30), cards(44), cards(9)
TO_THE_RIVER = [OPEN2, CALL, DRAW, CHECK, CHECK, DRAW, CHECK, CHECK, DRAW, CHECK, POT]  # seat 1 to answer a river bet
TO_THE_FLOP = [OPEN2, CALL, DRAW]
FLOP_ENTRY = Frontier(HOLES, 0, [FLOP], TO_THE_FLOP)
J = np.arange(MAX_HOLES)
SPREAD = (J % 4).astype(np.uint8)  # every world has members
EVEN = np.array([0.4, 0.3, 0.2, 0.1], F)
# (name, entry, hole_world, weights, origin); origin None = RP_NLHE_SUBGAME_ORIGIN_NONE
CASES = [
    ("river, seat 1", Frontier(HOLES, 1, [FLOP, TURN, RIVER], TO_THE_RIVER, [CHECK, POT]), SPREAD, EVEN, None),
    ("flop", FLOP_ENTRY, SPREAD, EVEN, None),
    ("flop, origin 0", FLOP_ENTRY, SPREAD, EVEN, 0),
    ("bad edge", Frontier(HOLES, 0, [FLOP], TO_THE_FLOP + [25]), SPREAD, EVEN, 0),
    ("preflop", Frontier(HOLES, 0), SPREAD, EVEN, -1),
    ("no other hole", Frontier((0, HOLES[1]), 1, [FLOP], TO_THE_FLOP + [CHECK], [CHECK]), SPREAD, EVEN, 0),
    ("a NaN weight", FLOP_ENTRY, SPREAD, np.array([0.5, NAN, 0.25, 0.25], F), None),
    ("a zero weight", FLOP_ENTRY, SPREAD, np.array([0.5, 0.0, 0.5, 0.0], F), 0),
    ("byte 77", FLOP_ENTRY, np.where(J % 5 == 0, 77, SPREAD).astype(np.uint8), EVEN, None),
    ("bad origin", FLOP_ENTRY, SPREAD, EVEN, 5),
    ("chance", Frontier(HOLES, 0, edges=[OPEN2, CALL], prefix=[OPEN2, CALL]), SPREAD, EVEN, -1),
    ("terminal", Frontier(HOLES, 0, edges=[OPEN2, FOLD], prefix=[OPEN2, FOLD]), SPREAD, EVEN, None),
    ("bad hole", Frontier((cards(51), HOLES[1]), 0, [FLOP], TO_THE_FLOP), SPREAD, EVEN, None),
]
NAMES = [c[0] for c in CASES]
STATUS = {"bad edge": FM.EDGE, "a NaN weight": FM.CARDS, "bad origin": FM.SEAT, "bad hole": FM.CARDS}
SHAPES = [(1, 2), (2, 2), (8, 2), (1, 1), (2, 1)]  # (iterations, rollouts)
# world 2 has all the weight and no member: every iteration is drawn to it and takes the fallback (two iterations: the model walks
# 10 000 attempts for each)
EMPTY_WORLD = (np.where(SPREAD == 2, 0, SPREAD).astype(np.uint8), np.array([0.0, 0.0, 1.0, 0.0], F))


class Model:
    def __init__(self):
        self.bp, self.want, self.solves = DM.Blueprint(), {}, {}
        self.kw = dict(bp_epoch=EPOCH, bias=BIAS, prior=PRIOR, seed=SEED, first_id=FIRST_ID)
        for rollouts, stops in ((2, (1, 2, 8)), (1, (1, 2))):
            for i, (name, entry, hole_world, weights, origin) in enumerate(CASES):
                try:
                    if origin is not None and not -1 <= origin <= 3:
                        raise SM.Malformed(FM.SEAT)
                    s = SM.Solve(entry, hole_world, weights, origin, self.bp, i, rollouts=rollouts, **self.kw)
                    self.solves[(rollouts, i)] = s
                    for t in range(max(stops)):
                        s.step()
                        if t + 1 in stops:
                            self.want[(t + 1, rollouts, i)] = s.harvest()
                except SM.Malformed as m:
                    for t in stops:
                        self.want[(t, rollouts, i)] = SM.failed(m.status)
        self.empty_world = [SM.solve(FLOP_ENTRY, *belief, 0, self.bp, i, 2, rollouts=1, **self.kw) for i, belief in enumerate((EMPTY_WORLD, (SPREAD, EVEN)))]
        self.table = self.bp.table()
        self.cap_log2 = (2 * self.table[0].size).bit_length()

    def solver(self):
        s = NlheSolver(cap_log2=self.cap_log2, batch=1, seed=1)
        s.load(*self.table, epoch=EPOCH)
        return s


@pytest.fixture(scope="module")
def model():
    return Model()


def entries(cases=CASES):
    return [c[1] for c in cases]


def beliefs(cases=CASES):
    return np.stack([c[2] for c in cases]), np.stack([c[3] for c in cases])


def origins(cases=CASES):
    return [c[4] for c in cases]


def assert_equal(res, rows, deals, want, name):
    """one solve's result, exported rows and traced deals against the model's harvest"""
    for f in ("status", "past", "present", "choices", "n_actions", "iterations", "n_rows", "nodes", "infosets", "frontiers", "rollouts", "attempts", "fallbacks"):
        assert int(res[f]) == int(want[f]), (name, f, int(res[f]), int(want[f]))
    assert np.array_equal(res["visits"], want["visits"]) and list(res["drawn"]) == want["drawn"], name
    for f in ("refined", "regret", "sum_regret"):
        assert np.array_equal(bits(res[f]), bits(want[f])), (name, f, res[f], want[f])
    assert want["n_rows"] <= ROWS_CAP, (name, want["n_rows"])
    for x, (world, kind, n_actions, past, present, choices, enc) in enumerate(want["rows"]):
        r = rows[x]
        got = (int(r["world"]), int(r["kind"]), int(r["n_actions"]), int(r["past"]), int(r["present"]), int(r["choices"]))
        assert got == (world, kind, n_actions, past, present, choices), (name, x)
        assert r["enc"].tobytes() == enc.tobytes(), (name, x, r["enc"], enc)
    assert not rows[want["n_rows"]:].view(np.uint8).any(), name
    traced = [(int(d["hole"]), int(d["world"]), int(d["attempts"])) for d in deals[: len(want["deals"])]]
    assert traced == want["deals"][: len(deals)] and not deals[len(want["deals"]):].view(np.uint8).any(), name


def solve(s, iterations, rollouts, cases=CASES, first_id=FIRST_ID, **kw):
    kw = dict(dict(rows_cap=ROWS_CAP, deals_cap=DEALS_CAP), **kw)
    return s.subgame_solve(entries(cases), beliefs(cases), origins(cases), iterations, rollouts, BIAS, PRIOR, SEED, first_id, **kw)


def test_every_case_occurs(model):
    """checked on the model, on the CPU, before anything is asked of the device: a fixture that does not meet these hides things"""
    m = model
    for i, name in enumerate(NAMES):
        for it, ro in SHAPES:
            assert m.want[(it, ro, i)]["status"] == STATUS.get(name, FM.OK), (name, it, ro)
    eight = {name: m.want[(8, 2, i)] for i, name in enumerate(NAMES)}
    for name in ("flop", "flop, origin 0"):
        assert len({r[0] for r in eight[name]["rows"]}) >= 3, name  # local rows in at least three distinct worlds
    # a world in which `internal`'s entry infoset has no local row: the harvest of that world falls to the blueprint
    flop = eight["flop"]
    entry_rows = {r[0] for r in flop["rows"] if (r[1], r[3], r[4], r[5]) == (SM.GAME, flop["past"], flop["present"], flop["choices"])}
    assert 0 < len(entry_rows) < 4 and flop["n_actions"] == 7
    assert eight["flop"]["rollouts"] == 0 and eight["flop"]["frontiers"] == 0 and eight["flop"]["n_rows"] > 8
    assert eight["river, seat 1"]["frontiers"] == 0 and eight["river, seat 1"]["n_rows"] > 0 and eight["river, seat 1"]["n_actions"] > 1
    assert eight["flop, origin 0"]["frontiers"] > 8 and eight["preflop"]["frontiers"] > 8 and eight["no other hole"]["frontiers"] > 0
    assert eight["flop, origin 0"]["n_rows"] > 64, "no profile past the rows kept in LDS"
    for name in ("flop, origin 0", "preflop", "no other hole"):
        assert any(r[1] == SM.PICK for r in eight[name]["rows"]) and any(r[1] == SM.GAME for r in eight[name]["rows"]), name
    assert eight["a zero weight"]["drawn"][1] == eight["a zero weight"]["drawn"][3] == 0 and min(eight["a zero weight"]["drawn"][0::2]) > 0
    assert {r[0] for r in eight["a zero weight"]["rows"]} == {0, 2}
    assert eight["byte 77"]["attempts"] > 0 and all(d[0] and SM.candidate(m.solves[(2, NAMES.index("byte 77"))].free, d[0]) % 5 for d in eight["byte 77"]["deals"])
    assert eight["chance"]["n_actions"] == 0 and eight["chance"]["frontiers"] == 8 and sum(eight["chance"]["drawn"]) == 8
    assert eight["terminal"]["n_actions"] == 0 and eight["terminal"]["nodes"] == 8 and eight["terminal"]["n_rows"] == 0
    assert all(sum(w["drawn"]) == w["iterations"] for w in m.want.values())
    assert any(d[2] > 0 for w in eight.values() for d in w["deals"]), "no deal was ever rejected"
    seen = [x for s in m.solves.values() for x in s.profile.seen]
    assert any(found for _, found in seen) and any(not found for _, found in seen)  # found and absent blueprint rows
    empty, usual = m.empty_world
    assert empty["status"] == usual["status"] == FM.OK and empty["drawn"] == [0, 0, 2, 0]
    assert empty["fallbacks"] == 2 and empty["attempts"] == 2 * SM.MAX_REJECTIONS and usual["fallbacks"] == 0 and usual["n_rows"] > 0


@pytest.mark.parametrize("iterations,rollouts", SHAPES)
def test_host_form_against_the_model(gpu, model, iterations, rollouts):
    m = model
    s = m.solver()
    res, rows, deals = solve(s, iterations, rollouts)
    for i, name in enumerate(NAMES):
        assert_equal(res[i], rows[i], deals[i], m.want[(iterations, rollouts, i)], name)


def test_a_world_without_a_member_takes_the_fallback(gpu, model):
    """legal as data: world 2 is drawn and no candidate belongs to it, so every such deal is the unconstrained attempt 10 000"""
    s = model.solver()
    hw, wt = np.stack([EMPTY_WORLD[0], SPREAD]), np.stack([EMPTY_WORLD[1], EVEN])
    res, rows, deals = s.subgame_solve([FLOP_ENTRY, FLOP_ENTRY], (hw, wt), 0, 2, 1, BIAS, PRIOR, SEED, FIRST_ID, ROWS_CAP, DEALS_CAP)
    for i, want in enumerate(model.empty_world):
        assert_equal(res[i], rows[i], deals[i], want, i)
    assert int(res[0]["fallbacks"]) == 2 and int(res[0]["attempts"]) == 2 * SM.MAX_REJECTIONS and (deals[0]["attempts"][:2] == SM.MAX_REJECTIONS).all()


def test_device_form_chained_from_the_belief(gpu, model):
    """rp_nlhe_belief_device -> rp_nlhe_subgame_solve_device without a host copy; every traced deal is rp_nlhe_restrict's deal t of 4 096
    for the same recall, seed and first_id; the host form on the same belief answers the same bytes; and the model agrees"""
    m = model
    s = m.solver()
    cases = [c for c in CASES if c[0] in ("river, seat 1", "flop", "flop, origin 0", "preflop", "no other hole", "chance")]
    en = NlheSolver.depth_entries(entries(cases))
    recalls = NlheSolver.subgame_recalls(en)
    og = NlheSolver._origin(origins(cases), len(cases), ORIGIN_NONE)
    bel = s.belief_device(torch.from_numpy(recalls.view(np.uint8).copy()).to("cuda"))
    dev = s.subgame_solve_device(torch.from_numpy(en.view(np.uint8).copy()).to("cuda"), bel["hole_world"], bel["weights"],
                                 torch.from_numpy(og).to("cuda"), 8, 2, BIAS, PRIOR, SEED, FIRST_ID, ROWS_CAP, DEALS_CAP)
    s.sync()
    assert all(t.is_cuda for t in dev) and not bel["status"].cpu().numpy().any()
    res = dev[0].cpu().numpy().view(SUBGAME_RESULT_DTYPE).reshape(-1)
    rows = dev[1].cpu().numpy().view(SUBGAME_ROW_DTYPE).reshape(len(cases), ROWS_CAP)
    deals = dev[2].cpu().numpy().view(SUBGAME_DEAL_DTYPE).reshape(len(cases), DEALS_CAP)
    assert not res["status"].any() and (res["iterations"] == 8).all()
    dealt = s.restrict(recalls, 4096, None, SEED, FIRST_ID)
    assert not dealt["status"].any()
    assert np.array_equal(deals["hole"], dealt["holes"][:, :DEALS_CAP]) and np.array_equal(deals["world"], dealt["world"][:, :DEALS_CAP])
    assert np.array_equal(deals["attempts"], dealt["attempts"][:, :DEALS_CAP])
    assert all(list(r["drawn"]) == [int((w[:8] == k).sum()) for k in range(4)] for r, w in zip(res, dealt["world"]))
    hw, wt = bel["hole_world"].cpu().numpy(), bel["weights"].cpu().numpy()
    host = s.subgame_solve(en, (hw, wt), origins(cases), 8, 2, BIAS, PRIOR, SEED, FIRST_ID, ROWS_CAP, DEALS_CAP)
    assert host[0].tobytes() == res.tobytes() and host[1].tobytes() == rows.tobytes() and host[2].tobytes() == deals.tobytes()
    i = [c[0] for c in cases].index("flop, origin 0")
    want = SM.solve(cases[i][1], hw[i], wt[i], 0, Table(*s.export()), i, 2, rollouts=2, **m.kw)
    two = s.subgame_solve(en, (hw, wt), origins(cases), 2, 2, BIAS, PRIOR, SEED, FIRST_ID, ROWS_CAP, DEALS_CAP)
    assert_equal(two[0][i], two[1][i], two[2][i], want, "flop, origin 0, the device's belief")


def test_a_history_past_the_cap_is_a_status(gpu, model):
    """the depth test's 47-edge entry between two valid ones, under a belief of rp_nlhe_belief: its tree is built and dealt for, its
    first frontier lies past RP_NLHE_MAX_HISTORY, so the solve ends with RP_RECALL_LENGTH — a zero result, zero rows, zero deals — and
    its neighbours answer what the model does"""
    m = model
    s = m.solver()
    # the record carries all three draws: the model deals through the recall's replay, which wants a card for every Draw edge it counts
    # (up to three), while the entry state itself stays on the flop — a Draw edge met at a choice node changes nothing
    long_entry = Frontier(HOLES, 0, [FLOP, TURN, RIVER], TO_THE_FLOP + [DRAW] * 44, prefix=[CHECK])
    flop_next = Frontier(HOLES, 0, [FLOP], TO_THE_FLOP, prefix=[CHECK])
    batch, rows_cap, deals_cap = [flop_next, long_entry, FLOP_ENTRY], 8, 2
    assert DM.street(FM.frontier_game(long_entry)) == 1 and len(long_entry.edges) == 47
    # the belief of the same seat, hole and flop three edges in: the candidate holes of the entry state
    bel = s.belief(NlheSolver.subgame_recalls([flop_next, flop_next, FLOP_ENTRY]))
    assert not bel["status"].any()
    table, keep = Table(*s.export()), []
    kw = dict(m.kw, rollouts=1)
    want = [SM.solve(e, bel["hole_world"][i], bel["weights"][i], 0, table, i, 2, keep=keep if e is long_entry else None, **kw)
            for i, e in enumerate(batch)]
    # on the model first: the entry itself replays, iteration 0 deals and builds a tree, and a frontier of that tree is what fails
    failed = keep[0]
    assert [w["status"] for w in want] == [FM.OK, FM.LENGTH, FM.OK] and failed.profile.t == 0 and len(failed.deals) == 1
    _, frontiers = failed.build(0)
    assert frontiers and all(len(long_entry.edges) + len(f.story) > FM.RM.MAX_HISTORY for f in frontiers)
    assert want[0]["frontiers"] > 0 and want[0]["n_rows"] > rows_cap and want[2]["n_rows"] > rows_cap
    res, rows, deals = s.subgame_solve(batch, bel, 0, 2, 1, BIAS, PRIOR, SEED, FIRST_ID, rows_cap, deals_cap)
    for i in range(3):
        assert_equal(res[i], rows[i], deals[i], dict(want[i], rows=want[i]["rows"][:rows_cap]), i)
    zero = np.zeros(1, SUBGAME_RESULT_DTYPE)
    zero["status"] = FM.LENGTH
    assert res[1].tobytes() == zero.tobytes() and not rows[1].view(np.uint8).any() and not deals[1].view(np.uint8).any()


def test_splits_repeats_and_reads_only(gpu, model):
    m = model
    s = m.solver()
    as_map = lambda past, present, choices, enc: {(int(p), int(q), int(c)): enc[i].tobytes() for i, (p, q, c) in enumerate(zip(past, present, choices))}
    before = (as_map(*s.export()), s.epoch, s.counters())
    host = solve(s, 8, 2)
    # the batch in two calls with matching first_id; the same call again; fewer rows and deals exported than there are; none
    cut = 5
    first, second = solve(s, 8, 2, CASES[:cut]), solve(s, 8, 2, CASES[cut:], FIRST_ID + cut)
    assert all(np.concatenate([a, b]).tobytes() == h.tobytes() for a, b, h in zip(first, second, host))
    again = solve(s, 8, 2)
    assert all(a.tobytes() == h.tobytes() for a, h in zip(again, host))
    few = solve(s, 8, 2, rows_cap=3, deals_cap=2)
    assert few[0].tobytes() == host[0].tobytes() and few[1].tobytes() == np.ascontiguousarray(host[1][:, :3]).tobytes()
    assert few[2].tobytes() == np.ascontiguousarray(host[2][:, :2]).tobytes()
    none = solve(s, 8, 2, rows_cap=0, deals_cap=0)
    assert none[0].tobytes() == host[0].tobytes() and none[1].shape == (len(CASES), 0) and none[2].shape == (len(CASES), 0)
    # an 8-iteration solve starts as the 2-iteration one did: the same first deals
    two = solve(s, 2, 2)
    assert np.array_equal(two[2][:, :2], host[2][:, :2]) and not two[2][:, 2:].view(np.uint8).any()
    # another seed deals other holes and samples other trees
    other = s.subgame_solve(entries(), beliefs(), origins(), 8, 2, BIAS, PRIOR, SEED + 1, FIRST_ID, ROWS_CAP, DEALS_CAP)
    assert np.array_equal(other[0]["status"], host[0]["status"]) and other[0].tobytes() != host[0].tobytes()
    # origin == NULL for the whole batch is RP_NLHE_SUBGAME_ORIGIN_NONE for every solve
    null = s.subgame_solve(entries()[:3], tuple(b[:3] for b in beliefs()), None, 8, 2, BIAS, PRIOR, SEED, FIRST_ID, ROWS_CAP, DEALS_CAP)
    each = s.subgame_solve(entries()[:3], tuple(b[:3] for b in beliefs()), [None] * 3, 8, 2, BIAS, PRIOR, SEED, FIRST_ID, ROWS_CAP, DEALS_CAP)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(null, each)) and not null[0]["rollouts"].any()
    # read-only: the export as a map, the epoch and the counters; and the table still trains
    after = (as_map(*s.export()), s.epoch, s.counters())
    assert before == after and after[1:] == (EPOCH, (0, 0, m.table[0].size))
    s.step()
    assert s.epoch == EPOCH + 1


NS_CHUNK = 1024  # solves per launch: NS_CHUNK of robopoker_amd/csrc/nlmc.hip


def test_a_batch_past_one_launch_equals_its_split(gpu, model):
    """NS_CHUNK + 1 solves take a second launch: every pointer and first_id move on by NS_CHUNK.  One call equals, byte for byte, the
    first NS_CHUNK solves and the last one asked for in calls of their own with matching first_id, in the host and the device form;
    the beliefs are rp_nlhe_belief_device's over the cycled recalls."""
    s = model.solver()
    n, rows_cap, deals_cap = NS_CHUNK + 1, 4, 2
    cases = [c for c in CASES if c[0] in ("river, seat 1", "flop", "flop, origin 0", "preflop", "no other hole", "chance")]
    # the cases cycled so that the second launch's only solve is one with frontiers and rows
    pick = (np.arange(n) - NS_CHUNK + [c[0] for c in cases].index("flop, origin 0")) % len(cases)
    en, og = NlheSolver.depth_entries(entries(cases))[pick], NlheSolver._origin(origins(cases), len(cases), ORIGIN_NONE)[pick]
    bel = s.belief_device(torch.from_numpy(NlheSolver.subgame_recalls(en).view(np.uint8).copy()).to("cuda"))
    en_dev, og_dev = torch.from_numpy(en.view(np.uint8).reshape(n, -1).copy()).to("cuda"), torch.from_numpy(og).to("cuda")
    parts = ((slice(0, n), FIRST_ID), (slice(0, NS_CHUNK), FIRST_ID), (slice(NS_CHUNK, n), FIRST_ID + NS_CHUNK))
    dev = [s.subgame_solve_device(en_dev[at], bel["hole_world"][at], bel["weights"][at], og_dev[at], 1, 1, BIAS, PRIOR, SEED, fid, rows_cap, deals_cap)
           for at, fid in parts]
    s.sync()
    assert all(t.is_cuda for part in dev for t in part) and not bel["status"].cpu().numpy().any()
    back = lambda t, dtype, *shape: np.frombuffer(t.cpu().numpy().tobytes(), dtype).reshape(shape)
    dev = [(back(r, SUBGAME_RESULT_DTYPE, len(r)), back(w, SUBGAME_ROW_DTYPE, len(r), rows_cap), back(d, SUBGAME_DEAL_DTYPE, len(r), deals_cap))
           for r, w, d in dev]
    hw, wt = bel["hole_world"].cpu().numpy(), bel["weights"].cpu().numpy()
    host = [s.subgame_solve(en[at], (hw[at], wt[at]), og[at], 1, 1, BIAS, PRIOR, SEED, fid, rows_cap, deals_cap) for at, fid in parts]
    for form, (whole, head, tail) in (("host", host), ("device", dev)):
        assert whole[0].shape == (n,) and whole[1].shape == (n, rows_cap) and whole[2].shape == (n, deals_cap), form
        for f in SUBGAME_RESULT_DTYPE.names:
            assert np.concatenate([head[0][f], tail[0][f]]).tobytes() == whole[0][f].tobytes(), (form, f)
        assert all(np.concatenate([a, b]).tobytes() == w.tobytes() for a, b, w in zip(head, tail, whole)), form
    assert all(d.tobytes() == h.tobytes() for d, h in zip(dev[0], host[0]))
    # the last solve is a real one, and its id is what it draws from: under the first solve's id it is dealt another hole
    last = host[0][0][-1]
    assert last["status"] == FM.OK and last["nodes"] > 1 and last["frontiers"] > 0 and last["n_rows"] > 0 and host[0][2][-1]["hole"][0] != 0
    wrong = s.subgame_solve(en[NS_CHUNK:], (hw[NS_CHUNK:], wt[NS_CHUNK:]), og[NS_CHUNK:], 1, 1, BIAS, PRIOR, SEED, FIRST_ID, rows_cap, deals_cap)
    assert wrong[2].tobytes() != host[2][2].tobytes()


def test_one_frontier_equals_the_frontier_entry_point(gpu, model):
    """the payoffs the model took for one frontier of a tree are rp_nlhe_frontier_payoffs' for the record that carries THAT
    ITERATION's hole for the other seat, and the stated id"""
    m = model
    s = m.solver()
    solve_ = m.solves[(2, NAMES.index("flop, origin 0"))]
    log = solve_.frontier_log
    assert len(log) > 8 and len({record.holes[1] for record, _, _ in log}) > 2  # the holes of several deals, not the entry's
    for record, fid, pay in (log[0], log[-1]):
        assert record.holes[1] in {d[0] for d in solve_.deals}
        got, status = s.frontier_payoffs(record, BIAS, 2, SEED, fid)
        assert status[0] == FM.OK and np.array_equal(bits(got[0]), bits(pay))


def test_arguments(gpu):
    lib = _lib.load()
    s = NlheSolver(cap_log2=10, batch=4, seed=2)
    en = NlheSolver.depth_entries([Frontier(HOLES, 0, edges=[OPEN2, FOLD])])
    hw, wt = SPREAD.reshape(1, -1).copy(), EVEN.reshape(1, -1).copy()
    res, rows, deals = np.zeros(1, SUBGAME_RESULT_DTYPE), np.zeros((1, 2), SUBGAME_ROW_DTYPE), np.zeros((1, 2), SUBGAME_DEAL_DTYPE)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def args(**kw):
        a = _lib.NlheSubgameArgs()
        lib.rp_nlhe_subgame_args_default(C.byref(a))
        for k, v in kw.items():
            setattr(a, k, v)
        return C.byref(a)

    fn = lib.rp_nlhe_subgame_solve
    assert fn(s._h, 1, p(en), p(hw), p(wt), None, args(), p(res), None, None) == _lib.RP_OK
    assert res[0]["status"] == FM.OK and res[0]["n_actions"] == 0 and res[0]["nodes"] == 1 and res[0]["iterations"] == 1 and res[0]["drawn"].sum() == 1
    assert fn(s._h, 1, p(en), p(hw), p(wt), None, args(rows_cap=2), p(res), None, None) == _lib.RP_ERR_INVALID
    assert fn(s._h, 1, p(en), p(hw), p(wt), None, args(deals_cap=2), p(res), None, None) == _lib.RP_ERR_INVALID
    assert fn(s._h, 1, p(en), p(hw), p(wt), None, args(rows_cap=2, deals_cap=2), p(res), p(rows), p(deals)) == _lib.RP_OK
    assert deals[0][0]["hole"] != 0 and not deals[0][1:].view(np.uint8).any()
    for missing in range(4):
        ptrs = [p(en), p(hw), p(wt), p(res)]
        ptrs[missing] = None
        assert fn(s._h, 1, ptrs[0], ptrs[1], ptrs[2], None, args(), ptrs[3], None, None) == _lib.RP_ERR_INVALID
    # an empty table solves the root: every infoset reads as the defaults, in every world
    root, _, _ = s.subgame_solve(Frontier((HOLES[0], 0), 0), (hw, wt), -1, iterations=4, rollouts=1)
    assert root[0]["status"] == FM.OK and root[0]["n_actions"] == 7 and abs(float(root[0]["refined"].sum()) - 1.0) < 1e-6
    s.step()
    assert s.epoch == 1 and s.counters()[2] > 0

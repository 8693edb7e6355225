"""The depth-limited re-solve from the device-resident blueprint: rp_nlhe_depth_solve, host and _device forms, against the naive model of
tests/nlhe_depth_model.py (pinned by tests/test_nlhe_depth_model.py).  Results and every exported row are compared as integers and bit
patterns: there is no tolerance.

One batch mixes every kind of entry with malformed records between valid ones; the model is run once per module (rollouts 2 with the
harvest taken after 1, 2 and 6 iterations, rollouts 1 after 1 and 2, one entry at rollouts 17) over one blueprint decided key by key as
the model asks, which is then loaded into the table."""
import ctypes as C

import numpy as np
import pytest
import torch

import nlhe_depth_model as DM
import nlhe_rollout_model as FM
import oracle_nlhe as ON
from nlhe_solve_common import bits, cards
from robopoker_amd import _lib
from robopoker_amd.nlhe import DEPTH_RESULT_DTYPE, DEPTH_ROW_DTYPE, Frontier, NlheSolver

pytestmark = pytest.mark.gpu

OPEN2, OPEN3, POT, HALF = ON.Open(2), ON.Open(3), ON.RaiseOdds(1, 1), ON.RaiseOdds(1, 2)
DRAW, FOLD, CHECK, CALL, SHOVE = ON.E_DRAW, ON.E_FOLD, ON.E_CHECK, ON.E_CALL, ON.E_SHOVE
BIAS, PRIOR, SEED, FIRST_ID, EPOCH, ROWS_CAP = 5.0, 64.0, 0x5EED, 1000, 3, 48
HOLES, FLOP, TURN, RIVER = (cards(51, 50), cards(12, 25)), cards(3, 17, 30), cards(44), cards(9)
TO_THE_RIVER = [OPEN2, CALL, DRAW, CHECK, CHECK, DRAW, CHECK, CHECK, DRAW, CHECK, POT]  # 11 edges, seat 1 to answer a river bet
TO_THE_FLOP = [OPEN2, CALL, DRAW]
# (name, entry, origin); the absent entry comes first: its keys are never loaded, whoever else asks for them
CASES = [
    ("absent", Frontier((cards(0, 1), cards(20, 33)), 0, [cards(21, 22, 23)], [OPEN3, CALL, DRAW, CHECK], [CHECK]), 1),
    ("river", Frontier(HOLES, 1, [FLOP, TURN, RIVER], TO_THE_RIVER, [CHECK, POT]), 3),
    ("flop, next street", Frontier(HOLES, 0, [FLOP], TO_THE_FLOP), 0),
    ("overlapping holes", Frontier((cards(51, 50), cards(50, 25)), 0, edges=[OPEN2, CALL]), 0),
    ("flop, adapt_leaf", Frontier(HOLES, 0, [FLOP], TO_THE_FLOP), None),
    ("preflop", Frontier(HOLES, 0), -1),
    ("bad edge", Frontier(HOLES, 0, [FLOP], [OPEN2, CALL, DRAW, 25]), 0),
    ("internal 1", Frontier(HOLES, 1, [FLOP], TO_THE_FLOP + [CHECK], [CHECK]), 0),
    ("uneven stacks", Frontier(HOLES, 0, [FLOP], TO_THE_FLOP + [CHECK, HALF], [CHECK, HALF], stacks=(150, 90)), 0),
    ("all in", Frontier(HOLES, 1, edges=[SHOVE], prefix=[SHOVE]), -1),
    ("bad origin", Frontier(HOLES, 0), 4),
    ("long prefix", Frontier(HOLES, 1, [FLOP, TURN, RIVER], TO_THE_RIVER, TO_THE_RIVER), 2),
    ("chance", Frontier(HOLES, 0, edges=[OPEN2, CALL], prefix=[OPEN2, CALL]), -1),
    ("terminal", Frontier(HOLES, 0, edges=[OPEN2, FOLD], prefix=[OPEN2, FOLD]), -1),
]
NAMES = [c[0] for c in CASES]
STATUS = {"overlapping holes": FM.CARDS, "bad edge": FM.EDGE, "bad origin": FM.SEAT}
FLOP_NEXT = Frontier(HOLES, 0, [FLOP], TO_THE_FLOP, prefix=[CHECK])
STRIDE = Frontier(HOLES, 0, [FLOP], TO_THE_FLOP)  # rollouts = 17: 272 games per frontier, more than one pass of the workgroup
SHAPES = [(1, 2), (2, 2), (6, 2), (1, 1), (2, 1)]  # (iterations, rollouts)


class Model:
    def __init__(self):
        self.bp, self.want, self.solves = DM.Blueprint(), {}, {}
        kw = dict(bp_epoch=EPOCH, bias=BIAS, prior=PRIOR, seed=SEED, first_id=FIRST_ID)
        for rollouts, stops in ((2, (1, 2, 6)), (1, (1, 2))):
            for i, (name, entry, origin) in enumerate(CASES):
                self.bp.forbid = name == "absent"
                try:
                    if origin is None:
                        origin = DM.street(FM.frontier_game(entry))
                    if not -1 <= origin <= 3:
                        raise DM.Malformed(FM.SEAT)
                    s = DM.Solve(entry, origin, self.bp, i, rollouts=rollouts, **kw)
                    self.solves[(rollouts, i)] = s
                    for t in range(max(stops)):
                        s.step()
                        if t + 1 in stops:
                            self.want[(t + 1, rollouts, i)] = s.harvest()
                except DM.Malformed as m:
                    for t in stops:
                        self.want[(t, rollouts, i)] = DM.failed(m.status)
            self.bp.forbid = False
        self.stride = DM.solve(STRIDE, 0, self.bp, 0, 1, rollouts=17, bp_epoch=EPOCH, bias=BIAS, prior=PRIOR, seed=SEED, first_id=7)
        self.table = self.bp.table()
        self.cap_log2 = (2 * self.table[0].size).bit_length()

    def solver(self):
        s = NlheSolver(cap_log2=self.cap_log2, batch=1, seed=1)
        s.load(*self.table, epoch=EPOCH)
        return s


@pytest.fixture(scope="module")
def model():
    return Model()


def entries():
    return [c[1] for c in CASES]


def origins():
    return [c[2] if c[0] != "bad origin" else 4 for c in CASES]


def assert_equal(res, rows, want, name):
    """one solve's result and exported rows against the model's harvest"""
    for f in ("status", "past", "present", "choices", "n_actions", "iterations", "n_rows", "nodes", "infosets", "frontiers", "rollouts"):
        assert int(res[f]) == int(want[f]), (name, f, int(res[f]), int(want[f]))
    assert np.array_equal(res["visits"], want["visits"]), name
    for f in ("refined", "regret", "sum_regret"):
        assert np.array_equal(bits(res[f]), bits(want[f])), (name, f, res[f], want[f])
    assert want["n_rows"] <= ROWS_CAP
    for x, (kind, n_actions, past, present, choices, enc) in enumerate(want["rows"]):
        r = rows[x]
        assert (int(r["kind"]), int(r["n_actions"]), int(r["past"]), int(r["present"]), int(r["choices"])) == (kind, n_actions, past, present, choices), (name, x)
        assert r["enc"].tobytes() == enc.tobytes(), (name, x, r["enc"], enc)
    assert not rows[want["n_rows"]:].view(np.uint8).any(), name


def solve(s, iterations, rollouts, **kw):
    return s.depth_solve(entries(), origins(), iterations, rollouts, BIAS, PRIOR, SEED, FIRST_ID, ROWS_CAP, **kw)


def test_every_case_occurs(model):
    m = model
    for i, name in enumerate(NAMES):
        for it, ro in SHAPES:
            assert m.want[(it, ro, i)]["status"] == STATUS.get(name, FM.OK), (name, it, ro)
    six = {name: m.want[(6, 2, i)] for i, name in enumerate(NAMES)}
    assert six["chance"]["n_actions"] == 0 and six["chance"]["frontiers"] == 6 and six["chance"]["n_rows"] == 1
    assert six["terminal"]["n_actions"] == 0 and six["terminal"]["nodes"] == 6 and six["terminal"]["n_rows"] == 0
    assert six["flop, adapt_leaf"]["rollouts"] == 0 and six["flop, adapt_leaf"]["n_rows"] > 2
    assert six["flop, next street"]["frontiers"] > 6 and six["preflop"]["frontiers"] > 6 and six["all in"]["frontiers"] > 0
    assert six["river"]["frontiers"] == 0 and six["river"]["n_rows"] > 0
    for name in ("flop, next street", "preflop", "internal 1", "uneven stacks"):
        assert any(r[0] == DM.PICK for r in six[name]["rows"]), name  # a Pick row
        assert any(r[0] == DM.GAME for r in six[name]["rows"]), name
    # found, absent and zero-weight blueprint rows; a warmstarted row whose blueprint row exists
    seen = [x for key, s in m.solves.items() for x in s.profile.seen]
    assert any(found for _, found in seen) and any(not found for _, found in seen)
    absent = m.solves[(2, NAMES.index("absent"))]
    assert absent.profile.seen and not any(found for _, found in absent.profile.seen) and six["absent"]["n_rows"] > 0
    loaded = {k: r for k, r in m.bp.loaded.items() if r is not None}
    assert any(not r["weight"][: DM.PM.nch(k[2])].any() for k, r in loaded.items()), "no all-zero row"
    assert any(r[0] == DM.GAME and (r[2], r[3], r[4]) in loaded for name in NAMES for r in six[name]["rows"]), "no warmstart from a found row"
    # the path saturates inside the tree of the long prefix: a node keyed with more than 12 story edges
    long_prefix = m.solves[(2, NAMES.index("long prefix"))]
    assert any(len(long_prefix.entry.prefix) + len(n.story) > FM.MAX_PREFIX for tree in long_prefix.trees for n in tree if n.kids)
    assert m.stride["status"] == FM.OK and m.stride["rollouts"] == m.stride["frontiers"] * 16 * 17 > 0


@pytest.mark.parametrize("iterations,rollouts", SHAPES)
def test_host_form_against_the_model(gpu, model, iterations, rollouts):
    m = model
    s = m.solver()
    res, rows = solve(s, iterations, rollouts)
    for i, name in enumerate(NAMES):
        assert_equal(res[i], rows[i], m.want[(iterations, rollouts, i)], name)


def test_more_rollouts_than_lanes(gpu, model):
    s = model.solver()
    res, rows = s.depth_solve(STRIDE, 0, 1, 17, BIAS, PRIOR, SEED, 7, ROWS_CAP)
    assert_equal(res[0], rows[0], model.stride, "stride")


def test_device_form_splits_repeats_and_reads_only(gpu, model):
    m = model
    s = m.solver()
    as_map = lambda past, present, choices, enc: {(int(p), int(q), int(c)): enc[i].tobytes() for i, (p, q, c) in enumerate(zip(past, present, choices))}
    before = (as_map(*s.export()), s.epoch, s.counters())
    host = solve(s, 6, 2)
    en = torch.from_numpy(NlheSolver.depth_entries(entries()).view(np.uint8).copy()).to("cuda")
    og = torch.from_numpy(NlheSolver._origin(origins(), len(CASES))).to("cuda")
    dev = s.depth_solve_device(en, og, 6, 2, BIAS, PRIOR, SEED, FIRST_ID, ROWS_CAP)
    s.sync()
    assert all(t.is_cuda for t in dev)
    assert dev[0].cpu().numpy().tobytes() == host[0].tobytes() and dev[1].cpu().numpy().tobytes() == host[1].tobytes()
    # the batch in two calls with matching first_id; the same call again; fewer rows exported than there are
    cut = 5
    first = s.depth_solve(entries()[:cut], origins()[:cut], 6, 2, BIAS, PRIOR, SEED, FIRST_ID, ROWS_CAP)
    second = s.depth_solve(entries()[cut:], origins()[cut:], 6, 2, BIAS, PRIOR, SEED, FIRST_ID + cut, ROWS_CAP)
    assert all(np.concatenate([a, b]).tobytes() == h.tobytes() for a, b, h in zip(first, second, host))
    again = solve(s, 6, 2)
    assert again[0].tobytes() == host[0].tobytes() and again[1].tobytes() == host[1].tobytes()
    few = s.depth_solve(entries(), origins(), 6, 2, BIAS, PRIOR, SEED, FIRST_ID, 3)
    assert few[0].tobytes() == host[0].tobytes() and few[1].tobytes() == np.ascontiguousarray(host[1][:, :3]).tobytes()
    none = s.depth_solve(entries(), origins(), 6, 2, BIAS, PRIOR, SEED, FIRST_ID, 0)
    assert none[0].tobytes() == host[0].tobytes() and none[1].shape == (len(CASES), 0)
    # another seed samples other trees
    other = s.depth_solve(entries(), origins(), 6, 2, BIAS, PRIOR, SEED + 1, FIRST_ID, ROWS_CAP)
    assert np.array_equal(other[0]["status"], host[0]["status"]) and other[0].tobytes() != host[0].tobytes()
    # read-only: the export as a map, the epoch and the counters; and the table still trains
    after = (as_map(*s.export()), s.epoch, s.counters())
    assert before == after and after[1:] == (EPOCH, (0, 0, m.table[0].size))
    s.step()
    assert s.epoch == EPOCH + 1


ND_CHUNK = 4096  # solves per launch: ND_CHUNK of robopoker_amd/csrc/nlmc.hip


@pytest.mark.parametrize("rows_cap", [0, 4])
def test_a_batch_past_one_launch_equals_its_split(gpu, model, rows_cap):
    """ND_CHUNK + 1 solves take a second launch: every pointer and first_id move on by ND_CHUNK.  One call equals, byte for byte, the
    first ND_CHUNK solves and the last one asked for in calls of their own with matching first_id, in the host and the device form."""
    s = model.solver()
    n = ND_CHUNK + 1
    # the cases cycled so that the second launch's only solve is one with frontiers and rows
    pick = (np.arange(n) - ND_CHUNK + NAMES.index("flop, next street")) % len(CASES)
    en, og = NlheSolver.depth_entries(entries())[pick], NlheSolver._origin(origins(), len(CASES))[pick]
    parts = ((slice(0, n), FIRST_ID), (slice(0, ND_CHUNK), FIRST_ID), (slice(ND_CHUNK, n), FIRST_ID + ND_CHUNK))
    host = [s.depth_solve(en[at], og[at], 1, 1, BIAS, PRIOR, SEED, fid, rows_cap) for at, fid in parts]
    en_dev, og_dev = torch.from_numpy(en.view(np.uint8).reshape(n, -1).copy()).to("cuda"), torch.from_numpy(og).to("cuda")
    dev = [s.depth_solve_device(en_dev[at], og_dev[at], 1, 1, BIAS, PRIOR, SEED, fid, rows_cap) for at, fid in parts]
    s.sync()
    assert all(t.is_cuda for pair in dev for t in pair)
    back = lambda t, dtype, *shape: np.frombuffer(t.cpu().numpy().tobytes(), dtype).reshape(shape)
    dev = [(back(r, DEPTH_RESULT_DTYPE, len(r)), back(w, DEPTH_ROW_DTYPE, len(r), rows_cap)) for r, w in dev]
    for form, (whole, head, tail) in (("host", host), ("device", dev)):
        assert whole[0].shape == (n,) and whole[1].shape == (n, rows_cap), form
        for f in DEPTH_RESULT_DTYPE.names:
            assert np.concatenate([head[0][f], tail[0][f]]).tobytes() == whole[0][f].tobytes(), (form, f)
        assert np.concatenate([head[0], tail[0]]).tobytes() == whole[0].tobytes(), form
        assert np.concatenate([head[1], tail[1]]).tobytes() == whole[1].tobytes(), form
    assert dev[0][0].tobytes() == host[0][0].tobytes() and dev[0][1].tobytes() == host[0][1].tobytes()
    # the last solve is a real one, and its id is what it draws from: under the first solve's id it samples another tree
    last = host[0][0][-1]
    assert last["status"] == FM.OK and last["nodes"] > 1 and last["frontiers"] > 0 and last["n_rows"] > 0
    assert rows_cap == 0 or host[0][1][-1].view(np.uint8).any()
    assert s.depth_solve(en[ND_CHUNK:], og[ND_CHUNK:], 1, 1, BIAS, PRIOR, SEED, FIRST_ID, rows_cap)[0].tobytes() != host[2][0].tobytes()


def test_one_frontier_equals_the_frontier_entry_point(gpu, model):
    """the payoffs the model took for one frontier of a tree are rp_nlhe_frontier_payoffs' for the stated record and id"""
    m = model
    s = m.solver()
    log = m.solves[(2, NAMES.index("flop, next street"))].frontier_log
    assert len(log) > 6
    for record, fid, pay in (log[0], log[-1]):
        got, status = s.frontier_payoffs(record, BIAS, 2, SEED, fid)
        assert status[0] == FM.OK and np.array_equal(bits(got[0]), bits(pay))


def test_arguments(gpu):
    lib = _lib.load()
    s = NlheSolver(cap_log2=10, batch=4, seed=2)
    en = NlheSolver.depth_entries([Frontier(HOLES, 0, edges=[OPEN2, FOLD])])
    res, rows = np.zeros(1, DEPTH_RESULT_DTYPE), np.zeros((1, 2), DEPTH_ROW_DTYPE)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def args(**kw):
        a = _lib.NlheDepthArgs()
        lib.rp_nlhe_depth_args_default(C.byref(a))
        for k, v in kw.items():
            setattr(a, k, v)
        return C.byref(a)

    assert lib.rp_nlhe_depth_solve(s._h, 1, p(en), None, args(), p(res), None) == _lib.RP_OK
    assert res[0]["status"] == FM.OK and res[0]["n_actions"] == 0 and res[0]["nodes"] == 1 and res[0]["iterations"] == 1
    assert lib.rp_nlhe_depth_solve(s._h, 1, p(en), None, args(rows_cap=2), p(res), None) == _lib.RP_ERR_INVALID
    assert lib.rp_nlhe_depth_solve(s._h, 1, p(en), None, args(rows_cap=2), p(res), p(rows)) == _lib.RP_OK
    assert lib.rp_nlhe_depth_solve(s._h, 1, None, None, args(), p(res), None) == _lib.RP_ERR_INVALID
    assert lib.rp_nlhe_depth_solve(s._h, 1, p(en), None, args(), None, None) == _lib.RP_ERR_INVALID
    # an empty table solves the root: every infoset reads as the defaults
    root, _ = s.depth_solve(Frontier(HOLES, 0), -1, iterations=4, rollouts=1)
    assert root[0]["status"] == FM.OK and root[0]["n_actions"] == 7 and abs(float(root[0]["refined"].sum()) - 1.0) < 1e-6
    s.step()
    assert s.epoch == 1 and s.counters()[2] > 0


class StoryPath(DM.Solve):
    """NOT the rule: a solve whose rollouts start their story from prefix ++ the game edges to the frontier node instead of from the
    prefix.  Only used to make a blueprint hold the keys that mistake would ask for, so that a kernel making it reads rows, not absences."""

    def frontier_payoffs(self, node):
        f = self.entry
        record = Frontier(f.holes, f.internal, f.draws, tuple(f.edges) + tuple(node.story), (tuple(f.prefix) + tuple(node.story))[:FM.MAX_PREFIX],
                          f.stacks, f.dealer)
        fid = ((self.tree_id() * DM.MAX_FRONTIERS) + node.frontier) & DM.M64
        status, pay, _ = FM.payoffs(record, self.bp, 0, self.bias, self.rollouts, self.seed, fid)
        assert status == FM.OK
        self.frontier_log.append((record, fid, pay))
        return pay


class PathModel:
    """a flop entry with a 10-edge prefix — the 12-edge cut of a key falls inside the first rollout steps, or inside the tree's own edges
    if they were counted — over a blueprint with a row for EVERY key either path convention asks for"""

    def __init__(self):
        self.bp = DM.Blueprint(dense=True)
        self.entry = Frontier(HOLES, 0, [FLOP], TO_THE_FLOP, prefix=[OPEN2, CALL, DRAW, CHECK, HALF, CALL, DRAW, CHECK, CHECK, DRAW])
        kw = dict(bp_epoch=EPOCH, rollouts=2, bias=BIAS, prior=PRIOR, seed=SEED, first_id=FIRST_ID)
        self.wrong, self.right = StoryPath(self.entry, 0, self.bp, 0, **kw), DM.Solve(self.entry, 0, self.bp, 0, **kw)
        for s in (self.wrong, self.right):
            for _ in range(6):
                s.step()
        self.table = self.bp.table()
        self.cap_log2 = (2 * self.table[0].size).bit_length()


@pytest.fixture(scope="module")
def path_model():
    return PathModel()


def test_the_fixture_tells_the_two_paths_apart(path_model):
    m = path_model
    differ = [i for i, (a, b) in enumerate(zip(m.right.frontier_log, m.wrong.frontier_log)) if a[1] != b[1] or a[2].tobytes() != b[2].tobytes()]
    assert differ, "no payoff matrix depends on where the story starts"
    right, wrong = m.right.harvest(), m.wrong.harvest()
    assert len(differ) > len(m.right.frontier_log) // 2
    assert right["refined"].tobytes() != wrong["refined"].tobytes() and [r[5].tobytes() for r in right["rows"]] != [r[5].tobytes() for r in wrong["rows"]]
    assert all(r is not None for r in m.bp.loaded.values())


def test_rollouts_start_from_the_prefix(gpu, path_model):
    """every key has a row, so a rollout keyed by another path plays other games: result and rows are the prefix convention's"""
    m = path_model
    s = NlheSolver(cap_log2=m.cap_log2, batch=1, seed=1)
    s.load(*m.table, epoch=EPOCH)
    res, rows = s.depth_solve(m.entry, 0, 6, 2, BIAS, PRIOR, SEED, FIRST_ID, ROWS_CAP)
    assert_equal(res[0], rows[0], m.right.harvest(), "long prefix, dense blueprint")
    # and the matrices the model took are the frontier entry point's, over the same table
    for record, fid, pay in m.right.frontier_log[:3] + m.right.frontier_log[-3:]:
        got, status = s.frontier_payoffs(record, BIAS, 2, SEED, fid)
        assert status[0] == FM.OK and np.array_equal(bits(got[0]), bits(pay))


def test_a_profile_past_the_rows_kept_in_lds(gpu):
    """20 iterations of a flop solve leave more than the 64 rows a workgroup keeps in LDS: lookups, updates, the ranking and the export
    cross into the solve's overflow region"""
    bp = DM.Blueprint()
    want = DM.solve(STRIDE, 0, bp, 3, 20, rollouts=1, bp_epoch=EPOCH, bias=BIAS, prior=PRIOR, seed=SEED, first_id=FIRST_ID)
    assert want["status"] == FM.OK and 64 < want["n_rows"] <= 160
    table = bp.table()
    s = NlheSolver(cap_log2=(2 * table[0].size).bit_length(), batch=1, seed=1)
    s.load(*table, epoch=EPOCH)
    # the solve sits fourth in its batch: its overflow region is not the launch's first
    res, rows = s.depth_solve([Frontier(HOLES, 0, edges=[OPEN2, FOLD])] * 3 + [STRIDE], 0, 20, 1, BIAS, PRIOR, SEED, FIRST_ID, 160)
    for f in ("status", "past", "present", "choices", "n_actions", "iterations", "n_rows", "nodes", "infosets", "frontiers", "rollouts"):
        assert int(res[3][f]) == int(want[f]), f
    for f in ("refined", "regret", "sum_regret"):
        assert np.array_equal(bits(res[3][f]), bits(want[f])), f
    for x, (kind, n_actions, past, present, choices, enc) in enumerate(want["rows"]):
        r = rows[3][x]
        assert (int(r["kind"]), int(r["n_actions"]), int(r["past"]), int(r["present"]), int(r["choices"])) == (kind, n_actions, past, present, choices), x
        assert r["enc"].tobytes() == enc.tobytes(), x
    assert not rows[3][want["n_rows"]:].view(np.uint8).any() and (res[:3]["n_rows"] == 0).all() and not res["status"].any()


def test_a_history_past_the_cap_is_a_status(gpu):
    """a 47-edge entry (Draw edges met at a choice node change nothing and still count): every frontier of its tree lies two game edges
    further, past RP_NLHE_MAX_HISTORY, so the solve ends with RP_RECALL_LENGTH; under adapt_leaf the same entry has no frontier and solves"""
    entry = Frontier(HOLES, 0, [FLOP], TO_THE_FLOP + [DRAW] * 44, prefix=[CHECK])
    bp = DM.Blueprint()
    kw = dict(rollouts=1, bp_epoch=EPOCH, bias=BIAS, prior=PRIOR, seed=SEED, first_id=FIRST_ID)
    want = [DM.solve(entry, 0, bp, 0, 2, **kw), DM.solve(entry, None, bp, 1, 2, **kw), DM.solve(FLOP_NEXT, 0, bp, 2, 2, **kw)]
    assert [w["status"] for w in want] == [FM.LENGTH, FM.OK, FM.OK] and want[1]["n_rows"] > 0
    table = bp.table()
    s = NlheSolver(cap_log2=(2 * table[0].size).bit_length() + 1, batch=1, seed=1)
    s.load(*table, epoch=EPOCH)
    res, rows = s.depth_solve([entry, entry, FLOP_NEXT], [0, None, 0], 2, 1, BIAS, PRIOR, SEED, FIRST_ID, ROWS_CAP)
    for i in range(3):
        assert_equal(res[i], rows[i], want[i], i)


def test_the_rows_kept_are_the_first_in_rank_order(gpu):
    """rows_cap below, at and above n_rows: the export keeps the first rows_cap rows of the ranking and pads with zero bytes, and the
    result — sum_regret is folded over ALL rows in rank order — does not depend on how many rows leave"""
    bp = DM.Blueprint()
    want = DM.solve(FLOP_NEXT, 0, bp, 0, 2, rollouts=1, bp_epoch=EPOCH, bias=BIAS, prior=PRIOR, seed=SEED, first_id=FIRST_ID)
    n_rows = want["n_rows"]
    assert want["status"] == FM.OK and n_rows > 1
    table = bp.table()
    s = NlheSolver(cap_log2=(2 * table[0].size).bit_length() + 1, batch=1, seed=1)
    s.load(*table, epoch=EPOCH)
    results = []
    for rows_cap in (1, n_rows, n_rows + 3):
        res, rows = s.depth_solve(FLOP_NEXT, 0, 2, 1, BIAS, PRIOR, SEED, FIRST_ID, rows_cap)
        assert rows.shape == (1, rows_cap)
        assert_equal(res[0], rows[0], dict(want, rows=want["rows"][:rows_cap]), rows_cap)
        assert not rows[0][n_rows:].view(np.uint8).any() and rows[0][:n_rows].view(np.uint8).reshape(min(rows_cap, n_rows), -1).any(axis=1).all()
        results.append(res.tobytes())
    assert results[0] == results[1] == results[2]

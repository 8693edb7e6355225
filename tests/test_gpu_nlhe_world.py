"""Subgame worlds from the device-resident blueprint: rp_nlhe_partition, rp_nlhe_belief and rp_nlhe_restrict, host and _device forms,
against the naive model of tests/nlhe_world_model.py (pinned by tests/test_nlhe_world_model.py).  Bit patterns and plain integers
only: there is no tolerance.

The partition rows are built by hand, and each property a row is there for is asserted on the model first.  The recalls are the range
test's kinds (tests/test_gpu_nlhe_range.py): the root, a flop history from each seat, a river history longer than the 12 edges a Path
keeps, a recall none of whose infosets has a row, a recall whose every reach is zero, and two malformed recalls between valid ones,
on a 2^10-slot table that holds about half of the infosets the model asks for (chosen by a hash of the key)."""
import ctypes as C

import numpy as np
import pytest
import torch

import nlhe_policy_model as PM
import nlhe_range_model as RM
import nlhe_read_chunk as RC
import nlhe_world_model as WM
import oracle_nlhe as ON
from robopoker_amd import _lib
from robopoker_amd.nlhe import A, ENC_DTYPE, MAX_HOLES, MAX_REJECTIONS, WORLD_NONE, WORLDS, NlheSolver, Recall

pytestmark = pytest.mark.gpu

F = np.float32
NONE = WORLD_NONE
CAP_LOG2 = 10
SLOTS = 1 << CAP_LOG2
WEIGHTS = np.array([0.0, 1e-39, 1.0, 1e12], np.float32)  # 1e-39 is subnormal: below RP_EPSILON
OPEN2, OPEN3, POT, HALF = ON.Open(2), ON.Open(3), ON.RaiseOdds(1, 1), ON.RaiseOdds(1, 2)
DRAW, FOLD, CHECK, CALL = ON.E_DRAW, ON.E_FOLD, ON.E_CHECK, ON.E_CALL
DEALS, SEED, FIRST_ID = 64, 0x5EED, (1 << 64) - 3  # the deal ids of the batch wrap


def cards(*cs):
    return sum(1 << c for c in cs)


def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- partition alone
def row(masses, at=None):
    mass, seen = np.zeros(256, F), np.zeros(256, bool)
    for b, m in zip(at if at is not None else range(len(masses)), masses):
        mass[b], seen[b] = m, True
    return mass, seen


def spanning_row():
    """masses over 1e-30 .. 1e3 from a fixed seed, where float32 rounding of the running sums decides a boundary: 128 buckets share one
    mass v of 1e2 .. 1e3 and the others hold 1e-30 .. 1e-3, which the float32 sums absorb.  Exactly, the running sum after 32 k of the
    v falls short of k quarters of the total by a quarter of the small masses; in float32 it may not.  The seed is the first one at
    which the same scan in float64 puts some bucket into another world."""
    for seed in range(200):
        rng = np.random.default_rng(seed)
        masses = (10.0 ** rng.uniform(-30, -3, 256)).astype(F)
        masses[rng.permutation(256)[:128]] = F(10.0 ** rng.uniform(2, 3))
        world, _, _ = WM.partition(masses, np.ones(256, bool))
        if not np.array_equal(world, partition_f64(masses)):
            return seed, masses
    raise AssertionError("no seed below 200 makes float32 rounding decide a boundary")


def partition_f64(masses):
    """the same scan in float64 over all 256 buckets"""
    m = masses.astype(np.float64)
    order = sorted(range(256), key=lambda b: -m[b])
    total, world, index, acc = m.sum(), np.zeros(256, np.uint8), 0, 0.0
    for b in order:
        acc += m[b]
        world[b] = index
        if acc >= total / 4 * (index + 1) and index < 3:
            index += 1
    return world


def partition_rows():
    """[(name, mass, seen)]"""
    rows = [("4 3 2 1", *row([4, 3, 2, 1])), ("10 1", *row([10, 1])), ("all equal", np.ones(256, F), np.ones(256, bool))]
    rows.append(("ties straddle a boundary", *row([3, 1, 1, 1, 1, 1, 1, 1, 1, 1], at=[200, 5, 17, 3, 90, 91, 92, 250, 0, 1])))
    rows.append(("threshold met exactly", *row([2, 2, 2, 2], at=[9, 8, 7, 6])))
    rows.append(("one entry", *row([0.125], at=[255])))
    rows.append(("two entries", *row([1, 3], at=[0, 255])))
    rows.append(("zeros beside positives", *row([0, 5, 0, 1, 0, 0, 2, 0], at=[1, 2, 3, 100, 101, 102, 103, 254])))
    rows.append(("zero total", *row([0, 0, 0, 0, 0], at=[4, 5, 60, 61, 255])))
    rows.append(("no entry", np.zeros(256, F), np.zeros(256, bool)))
    mass, seen = row([5, 1, 2], at=[10, 20, 30])
    mass[11], mass[200] = 1e9, 7  # a mass where seen is 0 is no entry
    rows.append(("mass without seen", mass, seen))
    rows.append(("descending by bucket", np.arange(256, 0, -1).astype(F), np.ones(256, bool)))
    rows.append(("ascending by bucket", np.arange(1, 257).astype(F), np.ones(256, bool)))
    rows.append(("subnormal", *row([1e-45, 1e-45, 3e-45, 1e-39], at=[0, 128, 64, 32])))
    rows.append(("one dominates", *row([1e3] + [1e-30] * 9, at=range(20, 30))))
    seed, masses = spanning_row()
    rows.append((f"spanning, seed {seed}", masses, np.ones(256, bool)))
    return rows


def test_partition_rows(gpu):
    rows = partition_rows()
    want = {name: WM.partition(mass, seen) for name, mass, seen in rows}
    # what each row is there for, on the model
    w = want["4 3 2 1"]
    assert list(w[0][:4]) == [0, 1, 2, 3] and np.array_equal(bits(w[1]), bits([F(0.4), F(0.3), F(0.2), F(0.1)]))
    w = want["10 1"]
    assert list(w[0][:2]) == [0, 1] and not w[1][2:].any()
    assert [int((want["all equal"][0] == k).sum()) for k in range(4)] == [64] * 4
    w = want["ties straddle a boundary"][0]  # total 12, segment 3: the 3 closes world 0, then the nine ones go 3 / 3 / 3 in ascending b
    assert w[200] == 0 and [int(w[b]) for b in (0, 1, 3, 5, 17, 90, 91, 92, 250)] == [1, 1, 1, 2, 2, 2, 3, 3, 3]
    w = want["threshold met exactly"]  # accumulated == segment * (index + 1) at every entry: >= advances
    assert [int(w[0][b]) for b in (6, 7, 8, 9)] == [0, 1, 2, 3] and np.array_equal(bits(w[1]), bits([0.25] * 4))
    assert want["one entry"][0][255] == 0 and np.array_equal(bits(want["one entry"][1]), bits([1, 0, 0, 0]))
    assert (want["two entries"][0][255], want["two entries"][0][0]) == (0, 1)
    w = want["zeros beside positives"][0]  # the zero masses come last and land in the last world reached
    assert w[2] == 0 and len({int(w[b]) for b in (1, 3, 101, 102, 254)}) == 1 and w[1] == max(w[w != NONE])
    w = want["zero total"]
    assert w[2] == 0 and (w[0] != NONE).sum() == 5 and not w[0][w[0] != NONE].any() and np.array_equal(bits(w[1]), bits([0.25] * 4))
    assert (want["no entry"][0] == NONE).all() and np.array_equal(bits(want["no entry"][1]), bits([0.25] * 4))
    assert want["mass without seen"][0][11] == NONE and want["mass without seen"][2] == 8
    for name, mass, seen in rows:
        assert ((want[name][0] != NONE) == seen).all(), name

    s = NlheSolver(cap_log2=CAP_LOG2, batch=1, seed=1)
    mass, seen = np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows])
    world, weights = s.partition(mass, seen)
    for i, (name, _, _) in enumerate(rows):
        assert np.array_equal(world[i], want[name][0]), name
        assert np.array_equal(bits(weights[i]), bits(want[name][1])), name
    # the device form, and a seen array that is not 0 / 1
    dw, dwt = s.partition_device(torch.from_numpy(mass).to("cuda"), torch.from_numpy(seen.astype(np.uint8) * 7).to("cuda"))
    s.sync()
    assert dw.is_cuda and np.array_equal(dw.cpu().numpy(), world) and np.array_equal(bits(dwt.cpu().numpy()), bits(weights))


# ---------------------------------------------------------------------------------------------------------- belief and restrict
HOLE, FLOP, TURN, RIVER = cards(51, 50), cards(3, 17, 30), cards(44), cards(9)
LONG = [OPEN2, POT, CALL, DRAW, CHECK, CHECK, DRAW, CHECK, CHECK, DRAW, CHECK, POT, POT, POT, CALL]  # 15 edges, the river from edge 10 on
# (name, recall); the absent recall comes first: its keys are never loaded, whoever else asks for them
CASES = [
    ("absent", Recall(1, cards(0, 1), [cards(20, 21, 22)], [OPEN3, CALL, DRAW, CHECK, CHECK])),
    ("root", Recall(0, HOLE)),
    ("flop pov 0", Recall(0, HOLE, [FLOP], [OPEN2, CALL, DRAW, CHECK, HALF, CALL])),
    ("bad edge", Recall(0, HOLE, [FLOP], [OPEN2, CALL, DRAW, 25])),
    ("flop pov 1", Recall(1, HOLE, [FLOP], [OPEN2, CALL, DRAW, CHECK, HALF, CALL])),
    ("river", Recall(1, HOLE, [FLOP, TURN, RIVER], LONG)),
    ("hole on the flop", Recall(0, cards(3, 50), [FLOP], [OPEN2, CALL, DRAW, CHECK])),
    # a Draw edge at a choice node where the seat opposite pov acts: factor 0 for every candidate
    ("zero total", Recall(1, HOLE, [FLOP, TURN], [OPEN2, CALL, CHECK, DRAW, CHECK, DRAW, CHECK], stacks=(150, 90))),
]
NAMES = [c[0] for c in CASES]
STATUS = {"bad edge": RM.EDGE, "hole on the flop": RM.CARDS}
ZERO = NAMES.index("zero total")


class Rows:
    """the blueprint the model reads, decided key by key as the model asks (as the range test does it): about half of the keys get a
    row of corner weights, the others — and every key the absent recall asked for — have none"""

    def __init__(self):
        self.loaded, self.never, self.forbid, self.n_rows = {}, set(), False, 0

    def get(self, key):
        if self.forbid:
            self.never.add(key)
        if key in self.never:
            return None
        if key not in self.loaded:
            h = PM.key_hash(key[0] ^ 0x5EED, key[2], key[1])
            w = None
            if h % 2 == 0 and self.n_rows < SLOTS - 64:
                self.n_rows += 1
                w = WEIGHTS[[(h >> (8 + 2 * a)) & 3 for a in range(A)]].copy()
                if (h >> 40) % 8 == 0:
                    w[:] = 0.0
                w[PM.nch(key[2]):] = 7.0
            self.loaded[key] = w
        return self.loaded[key]

    def table(self):
        keys = [k for k, w in self.loaded.items() if w is not None]
        enc = np.zeros((len(keys), A), dtype=ENC_DTYPE)
        enc["weight"] = np.stack([self.loaded[k] for k in keys])
        enc["regret"], enc["payoff"], enc["visits"] = -3.0, 2.5, 11
        return (np.array([k[0] for k in keys], np.uint64), np.array([k[1] for k in keys], np.uint32),
                np.array([k[2] for k in keys], np.uint64), enc)


def requests():
    """worlds [n][DEALS]: 16 deals per world; the zero-total recall keeps its deals to worlds 1 - 3 (10 000 model attempts each) to a
    handful; one malformed request"""
    w = np.tile(np.repeat(np.arange(4, dtype=np.uint8), DEALS // 4), (len(CASES), 1))
    w[ZERO] = 0
    w[ZERO, [5, 20, 41]] = [1, 2, 3]
    w[NAMES.index("flop pov 0"), 7] = 9
    w[NAMES.index("root"), 63] = NONE  # "draw the world" among explicit requests
    return w


class Model:
    """the model's answers for CASES, computed once per module"""

    def __init__(self):
        self.rows, self.belief = Rows(), []
        for name, r in CASES:
            self.rows.forbid = name == "absent"
            self.belief.append(WM.belief(r, self.rows))
        self.rows.forbid = False
        self.table = self.rows.table()
        self.worlds = requests()
        self.stated = [WM.restrict(r, self.belief[i], i, DEALS, self.worlds[i], SEED, FIRST_ID) for i, (_, r) in enumerate(CASES)]
        self.drawn = [WM.restrict(r, self.belief[i], i, DEALS if i != ZERO else 4, None, SEED + 1, 0) for i, (_, r) in enumerate(CASES)]

    def solver(self, rows=None):
        s = NlheSolver(cap_log2=CAP_LOG2, batch=1, seed=1)
        s.load(*(x[:rows] for x in self.table), epoch=3)
        return s


@pytest.fixture(scope="module")
def model():
    return Model()


RECALLS = [c[1] for c in CASES]


def check_belief(got, j, want, what):
    assert got["status"][j] == want["status"], what
    assert np.array_equal(got["world"][j], want["world"]) and np.array_equal(bits(got["weights"][j]), bits(want["weights"])), what
    assert np.array_equal(got["hole_world"][j], want["hole_world"]), what


def check_deals(got, j, want, what):
    assert np.array_equal(got["holes"][j], want[0]), what
    assert np.array_equal(got["world"][j], want[1]) and np.array_equal(got["attempts"][j], want[2]), what


def test_the_model_exercises_every_case(model):
    m = model
    assert SLOTS // 2 < m.table[0].size < SLOTS
    for i, name in enumerate(NAMES):
        b = m.belief[i]
        assert b["status"] == STATUS.get(name, RM.OK), name
        assert (b["count"] > 0) == (b["status"] == RM.OK) and ((b["hole_world"] != NONE).sum() == b["count"]), name
    assert any(all((b["hole_world"] == w).any() for w in range(WORLDS)) for b in m.belief), "no recall has members in all four worlds"
    z = m.belief[ZERO]
    assert z["total"] == 0 and z["count"] > 0 and not z["hole_world"][: z["count"]].any() and np.array_equal(bits(z["weights"]), bits([0.25] * 4))
    absent = m.belief[NAMES.index("absent")]  # uniform reaches: the masses are small multiples of one value, ties everywhere
    assert len(np.unique(bits(absent["mass"][absent["seen"]]))) < absent["seen"].sum() // 2
    assert len(CASES[NAMES.index("river")][1].edges) > 12
    # restrict: the fallback where a world is empty, rejections elsewhere, the malformed request, drawn worlds of every kind
    holes, out, attempts = m.stated[ZERO]
    assert sorted(np.flatnonzero(attempts == MAX_REJECTIONS)) == [5, 20, 41] and not attempts[out == 0].any()
    others = [i for i in range(len(CASES)) if i != ZERO and m.belief[i]["status"] == RM.OK]
    assert any(m.stated[i][2].max() > 0 for i in others) and all(m.stated[i][2].max() < MAX_REJECTIONS for i in others)
    bad = NAMES.index("flop pov 0")
    assert (m.stated[bad][0][7], m.stated[bad][1][7], m.stated[bad][2][7]) == (0, NONE, 0)
    assert m.stated[NAMES.index("root")][1][63] < WORLDS
    assert len({int(w) for i in others for w in m.drawn[i][1]}) == WORLDS
    assert (m.drawn[ZERO][2] == MAX_REJECTIONS).any()
    for i in range(len(CASES)):
        r, b = RECALLS[i], m.belief[i]
        if b["status"] != RM.OK:
            assert all(not x[0].any() and (x[1] == NONE).all() and not x[2].any() for x in (m.stated[i], m.drawn[i])), NAMES[i]
            continue
        _, board, _ = RM.board_of(r, RM.validate(r))
        candidates = {h: j for j, h in enumerate(RM.hand_iterator(board | r.hole))}
        for holes, out, attempts in (m.stated[i], m.drawn[i]):
            for h, w, a in zip(holes, out, attempts):
                if w == NONE:
                    continue
                assert RM.popcount(int(h)) == 2 and int(h) in candidates, NAMES[i]  # two cards disjoint from pov's hole and the board
                assert a == MAX_REJECTIONS or b["hole_world"][candidates[int(h)]] == w, NAMES[i]


def test_belief(gpu, model):
    m = model
    s = m.solver()
    before = (s.export(), s.epoch, s.counters())
    got = s.belief(RECALLS)
    for i, name in enumerate(NAMES):
        check_belief(got, i, m.belief[i], name)
    # the same as the partition of the range query's own answer
    mass, seen, status = s.opponent_range(RECALLS)
    world, weights = s.partition(mass, seen)
    assert np.array_equal(status, got["status"]) and np.array_equal(world, got["world"]) and np.array_equal(bits(weights), bits(got["weights"]))
    for i in range(len(CASES)):
        assert np.array_equal(bits(mass[i]), bits(m.belief[i]["mass"])) and np.array_equal(seen[i], m.belief[i]["seen"])
    # hole_world and status may be NULL
    lib, rec = _lib.load(), Recall.pack(RECALLS)
    w2, wt2 = np.zeros((len(CASES), 256), np.uint8), np.zeros((len(CASES), WORLDS), F)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.rp_nlhe_belief(s._h, len(CASES), p(rec), p(w2), p(wt2), None, None) == _lib.RP_OK
    assert np.array_equal(w2, got["world"]) and np.array_equal(bits(wt2), bits(got["weights"]))
    # read-only
    after = (s.export(), s.epoch, s.counters())
    assert all(np.array_equal(x, y) for x, y in zip(before[0][:3], after[0][:3])) and before[0][3].tobytes() == after[0][3].tobytes()
    assert before[1:] == after[1:] == (3, (0, 0, m.table[0].size))


def test_restrict(gpu, model):
    m = model
    s = m.solver()
    got = s.restrict(RECALLS, DEALS, m.worlds, SEED, FIRST_ID)
    for i, name in enumerate(NAMES):
        assert got["status"][i] == m.belief[i]["status"], name
        check_deals(got, i, m.stated[i], name)
    # drawn worlds (worlds == NULL); the zero-total recall, most of whose draws fall back, with a handful of deals in a call of its own
    rest = [i for i in range(len(CASES)) if i != ZERO]
    drawn = s.restrict([RECALLS[i] for i in rest], DEALS, None, SEED + 1, 0)
    # `rest` leaves out the last recall only, so recall i of this call is CASES[i] with the same first_id + r
    assert rest == list(range(len(CASES) - 1))
    for j, i in enumerate(rest):
        check_deals(drawn, j, m.drawn[i], NAMES[i])
    check_deals(s.restrict(RECALLS[ZERO], 4, None, SEED + 1, ZERO), 0, m.drawn[ZERO], "zero total, drawn")
    # batch independence: one recall alone with first_id + r answers what it answered inside the batch
    for i in (NAMES.index("flop pov 1"), NAMES.index("river")):
        alone = s.restrict(RECALLS[i], DEALS, m.worlds[i], SEED, (FIRST_ID + i) & WM.M64)
        check_deals(alone, 0, m.stated[i], NAMES[i])
    # world_out, attempts and status may be NULL
    lib, rec = _lib.load(), Recall.pack(RECALLS)
    holes = np.zeros((len(CASES), DEALS), np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.rp_nlhe_restrict(s._h, len(CASES), p(rec), DEALS, p(m.worlds), SEED, FIRST_ID, p(holes), None, None, None) == _lib.RP_OK
    assert np.array_equal(holes, got["holes"])


def test_device_forms_equal_the_host_forms(gpu, model):
    m = model
    s = m.solver()
    rec = torch.from_numpy(Recall.pack(RECALLS).view(np.uint8).copy()).to("cuda")
    host, dev = s.belief(RECALLS), s.belief_device(rec)
    s.sync()
    assert all(t.is_cuda for t in dev.values())
    for f in ("world", "hole_world", "status"):
        assert np.array_equal(dev[f].cpu().numpy(), host[f]), f
    assert np.array_equal(bits(dev["weights"].cpu().numpy()), bits(host["weights"]))
    for worlds, seed in ((m.worlds, SEED), (None, SEED + 1)):
        host = s.restrict(RECALLS, DEALS, worlds, seed, FIRST_ID)
        dev = s.restrict_device(rec, DEALS, None if worlds is None else torch.from_numpy(worlds).to("cuda"), seed, FIRST_ID)
        s.sync()
        assert np.array_equal(dev["holes"].cpu().numpy().view(np.uint64), host["holes"])
        assert np.array_equal(dev["world"].cpu().numpy(), host["world"]) and np.array_equal(dev["status"].cpu().numpy(), host["status"])
        assert np.array_equal(dev["attempts"].cpu().numpy().view(np.uint16), host["attempts"])


def as_map(past, present, choices, enc):
    return {(int(p), int(q), int(c)): enc[i].tobytes() for i, (p, q, c) in enumerate(zip(past, present, choices))}


def test_a_queried_table_steps_like_one_never_queried(gpu, model):
    m = model
    s, twin = m.solver(rows=256), m.solver(rows=256)
    mass, seen, _ = s.opponent_range(RECALLS)
    s.partition(mass, seen)
    s.belief(RECALLS)
    s.restrict(RECALLS, 8, None, 1, 0)
    s.step()
    twin.step()
    # as maps by key: a step inserts from many lanes at once, so which slot a new infoset lands in differs from run to run
    am, bm = as_map(*s.export()), as_map(*twin.export())
    assert am.keys() == bm.keys() and len(am) > 256 and all(am[k] == bm[k] for k in am)
    assert (s.epoch, s.counters()) == (twin.epoch, twin.counters()) and s.epoch == 4


def hash_buckets(obs, street):
    """the hash encoder's bucket index of canonical observations (nl_bucket, encoder 0) for a whole isomorphism list"""
    u = np.uint64
    z = obs.astype(np.int64).view(np.uint64) ^ u((0x51ED270B5 * (street + 1)) & PM.M64)
    z ^= z >> u(30)
    z *= u(0xBF58476D1CE4E5B9)
    z ^= z >> u(27)
    z *= u(0x94D049BB133111EB)
    z ^= z >> u(31)
    return (z % u((169, 256, 256, 101)[street])).astype(np.uint8)


def test_a_world_with_no_member(gpu, model):
    # the encoder over rp_lookup tables, as the range test builds it, but the flop table holds TWO bucket values (the parity of the hash
    # encoder's): a flop belief has two entries, worlds 2 and 3 are empty while the total is positive, and their deals fall back.  The
    # turn table holds the isomorphisms of the first 16 pockets only: a recall that needs a turn bucket meets a hole it does not know
    from robopoker_amd import deuce

    tables = []
    for street, (name, pockets) in enumerate((("pref", 1326), ("flop", 1326), ("turn", 16), ("rive", 16))):
        obs = deuce.isomorphisms(name, 0, pockets)
        value = hash_buckets(obs.cpu().numpy(), street)
        tables.append(deuce.Lookup(name, obs, torch.from_numpy(value & 1 if street == 1 else value).to("cuda")))
    s = NlheSolver(cap_log2=CAP_LOG2, batch=1, seed=1, tables=tables)
    s.load(*model.table, epoch=3)
    # the subject's nodes are all before the flop (keyed through the pref table = the hash encoder's buckets); the head board is the flop
    r = Recall(0, HOLE, [FLOP], [OPEN2, CALL, DRAW])
    parity = lambda street, hole, board: WM.hash_bucket(street, hole, board) & 1
    want = WM.belief(r, model.rows, bucket=parity)
    assert want["status"] == RM.OK and want["total"] > 0 and want["seen"].sum() == 2
    assert [bool((want["hole_world"] == w).any()) for w in range(WORLDS)] == [True, True, False, False] and not want["weights"][2:].any()
    worlds = np.array([[0, 1, 2, 3, 3, 2, 1, 0]], np.uint8)
    deals = WM.restrict(r, want, 0, 8, worlds[0], 9, 100, bucket=parity)
    assert list(deals[2]) == [deals[2][0], deals[2][1], MAX_REJECTIONS, MAX_REJECTIONS, MAX_REJECTIONS, MAX_REJECTIONS, deals[2][6], deals[2][7]]
    assert max(deals[2][[0, 1, 6, 7]]) < MAX_REJECTIONS and all(RM.popcount(int(h)) == 2 and not int(h) & (HOLE | FLOP) for h in deals[0])
    lost = Recall(0, HOLE, [FLOP, TURN], [OPEN2, CALL, DRAW, CHECK, CHECK, DRAW])
    got = s.belief([r, lost])
    check_belief(got, 0, want, "two flop buckets")
    assert got["status"][1] == RM.LOOKUP and (got["world"][1] == NONE).all() and (got["hole_world"][1] == NONE).all()
    assert np.array_equal(bits(got["weights"][1]), bits([0.25] * 4))
    dealt = s.restrict([r, lost], 8, np.concatenate([worlds, worlds]), 9, 100)
    check_deals(dealt, 0, deals, "two flop buckets")
    assert dealt["status"][1] == RM.LOOKUP and not dealt["holes"][1].any() and (dealt["world"][1] == NONE).all() and not dealt["attempts"][1].any()
    s.close()
    for t in tables:
        t.close()


def test_arguments(gpu):
    lib = _lib.load()
    s = NlheSolver(cap_log2=CAP_LOG2, batch=4, seed=2)
    rec = Recall.pack([Recall(0, HOLE)])
    mass, seen = np.ones((1, 256), F), np.ones((1, 256), np.uint8)
    world, weights, holes = np.zeros((1, 256), np.uint8), np.zeros((1, WORLDS), F), np.zeros((1, 4), np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for fn in (lib.rp_nlhe_partition, lib.rp_nlhe_partition_device):
        assert fn(s._h, 0, None, None, None, None) == _lib.RP_OK
        assert fn(None, 1, p(mass), p(seen), p(world), p(weights)) == _lib.RP_ERR_INVALID
    for missing in range(4):
        args = [p(mass), p(seen), p(world), p(weights)]
        args[missing] = None
        assert lib.rp_nlhe_partition(s._h, 1, *args) == _lib.RP_ERR_INVALID and b"rp_nlhe_partition" in lib.rp_last_error()
    for fn in (lib.rp_nlhe_belief, lib.rp_nlhe_belief_device):
        assert fn(s._h, 0, None, None, None, None, None) == _lib.RP_OK
    assert lib.rp_nlhe_belief(s._h, 1, None, p(world), p(weights), None, None) == _lib.RP_ERR_INVALID
    assert lib.rp_nlhe_belief(s._h, 1, p(rec), None, p(weights), None, None) == _lib.RP_ERR_INVALID
    assert lib.rp_nlhe_belief(s._h, 1, p(rec), p(world), None, None, None) == _lib.RP_ERR_INVALID and b"rp_nlhe_belief" in lib.rp_last_error()
    for fn in (lib.rp_nlhe_restrict, lib.rp_nlhe_restrict_device):
        assert fn(s._h, 0, None, 4, None, 0, 0, None, None, None, None) == _lib.RP_OK  # n = 0
        assert fn(s._h, 1, None, 0, None, 0, 0, None, None, None, None) == _lib.RP_OK  # deals = 0
        assert fn(s._h, 1, p(rec), 4097, None, 0, 0, p(holes), None, None, None) == _lib.RP_ERR_INVALID and b"4096" in lib.rp_last_error()
    assert lib.rp_nlhe_restrict(s._h, 1, None, 4, None, 0, 0, p(holes), None, None, None) == _lib.RP_ERR_INVALID
    assert lib.rp_nlhe_restrict(s._h, 1, p(rec), 4, None, 0, 0, None, None, None, None) == _lib.RP_ERR_INVALID
    # an empty table answers the root: every reach is 1, the masses are the bucket sizes; 4 deals with drawn worlds
    assert lib.rp_nlhe_belief(s._h, 1, p(rec), p(world), p(weights), None, None) == _lib.RP_OK
    want = WM.belief(Recall(0, HOLE), {})
    assert np.array_equal(world[0], want["world"]) and np.array_equal(bits(weights[0]), bits(want["weights"]))
    assert lib.rp_nlhe_restrict(s._h, 1, p(rec), 4, None, 3, 0, p(holes), None, None, None) == _lib.RP_OK
    assert np.array_equal(holes[0], WM.restrict(Recall(0, HOLE), want, 0, 4, None, 3, 0)[0])
    # the most deals a call takes
    out = s.restrict(Recall(0, HOLE), 4096, None, 3, 0)
    assert np.array_equal(out["holes"][0, :4], holes[0])  # recall 0 of first_id 0: deal d has id d whatever `deals` is
    assert (out["world"] < WORLDS).all() and (out["attempts"] < MAX_REJECTIONS).all() and all(RM.popcount(int(h)) == 2 and not int(h) & HOLE for h in out["holes"][0, ::97])
    # a history longer than the cap is a status, not an error; the handle still steps
    long = Recall(0, HOLE, [FLOP], [CHECK] * 60)
    assert s.belief(long)["status"][0] == RM.LENGTH and s.restrict(long, 2)["status"][0] == RM.LENGTH and not s.restrict(long, 2)["holes"].any()
    s.step()
    assert s.epoch == 1 and s.counters()[2] > 0


# ---- the launch chunk (tests/nlhe_read_chunk.py): a batch cut into several launches answers what one launch answers ----
def from_device(s, out):
    s.sync()
    return {k: v.cpu().numpy() for k, v in out.items()} if isinstance(out, dict) else [v.cpu().numpy() for v in out]


def test_the_partition_does_not_depend_on_the_launch_chunk(gpu):
    rows = partition_rows()[1:]  # 15 rows: not a multiple of the staging arena's alignment
    n = len(rows)
    mass, seen = np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows])
    d_mass, d_seen = torch.from_numpy(mass).to("cuda"), torch.from_numpy(seen.astype(np.uint8)).to("cuda")
    s = NlheSolver(cap_log2=CAP_LOG2, batch=1, seed=1)
    with RC.read_chunk(None):
        want = s.partition(mass, seen)
    assert n % 16 and n >= 7
    for chunk in RC.cuts(n):
        with RC.read_chunk(chunk):
            host, dev = s.partition(mass, seen), from_device(s, s.partition_device(d_mass, d_seen))
        RC.same(host, want, (chunk, "host"))
        RC.same(dev, want, (chunk, "device"))
        for i, (name, row_mass, row_seen) in enumerate(rows):  # the model itself, on every row of every launch
            world, weights, _ = WM.partition(row_mass, row_seen)
            assert np.array_equal(host[0][i], world) and np.array_equal(bits(host[1][i]), bits(weights)), (chunk, name)
    with RC.read_chunk(1):
        RC.same(s.partition(mass[-1:], seen[-1:]), RC.tail(want, n - 1), "one row")


def test_the_belief_does_not_depend_on_the_launch_chunk(gpu, model):
    m, s = model, model.solver()
    n = len(RECALLS)
    rec = torch.from_numpy(Recall.pack(RECALLS).view(np.uint8).copy()).to("cuda")
    with RC.read_chunk(None):
        want = s.belief(RECALLS)
    assert n % 16 and n >= 7 and len(set(want["status"])) == 3
    for chunk in RC.cuts(n):
        with RC.read_chunk(chunk):
            host, dev = s.belief(RECALLS), from_device(s, s.belief_device(rec))
        RC.same(host, want, (chunk, "host"))
        RC.same(dev, want, (chunk, "device"))
        for i, name in enumerate(NAMES):  # the model itself; the zero-total recall is the last launch of n - 1
            check_belief(host, i, m.belief[i], (chunk, name))
    with RC.read_chunk(1):
        RC.same(s.belief(RECALLS[ZERO]), {k: v[ZERO: ZERO + 1] for k, v in want.items()}, "one recall")
    # hole_world and status left out, in launches of 3
    lib, packed = _lib.load(), Recall.pack(RECALLS)
    world, weights = np.zeros((n, 256), np.uint8), np.zeros((n, WORLDS), F)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    with RC.read_chunk(3):
        assert lib.rp_nlhe_belief(s._h, n, p(packed), p(world), p(weights), None, None) == _lib.RP_OK
    RC.same((world, weights), (want["world"], want["weights"]), "without hole_world and status")


@pytest.mark.parametrize("deals,columns", [(1, slice(7, 8)), (5, slice(3, 8))])
def test_the_deals_do_not_depend_on_the_launch_chunk(gpu, model, deals, columns):
    """the columns hold the malformed request of "flop pov 0" and, with 5 deals, the zero-total recall's request for an empty world"""
    m, s = model, model.solver()
    n = len(RECALLS)
    worlds = np.ascontiguousarray(m.worlds[:, columns])
    assert worlds.shape == (n, deals) and FIRST_ID and (worlds == 9).any() and (deals == 1 or worlds[ZERO].any())
    rec, d_worlds = torch.from_numpy(Recall.pack(RECALLS).view(np.uint8).copy()).to("cuda"), torch.from_numpy(worlds).to("cuda")
    call = lambda recalls, asked, first_id: s.restrict(recalls, deals, asked, SEED, first_id & WM.M64)
    with RC.read_chunk(None):
        want, drawn = call(RECALLS, worlds, FIRST_ID), call(RECALLS, None, FIRST_ID)
    for i, (name, r) in enumerate(CASES):  # one launch against the model at this number of deals: the ids are (first_id + r) * deals + d
        assert want["status"][i] == m.belief[i]["status"], name
        check_deals(want, i, WM.restrict(r, m.belief[i], i, deals, worlds[i], SEED, FIRST_ID), name)
    for chunk in RC.cuts(n):
        with RC.read_chunk(chunk):
            host = call(RECALLS, worlds, FIRST_ID)
            dev = from_device(s, s.restrict_device(rec, deals, d_worlds, SEED, FIRST_ID))
        RC.same(host, want, (chunk, "host"))
        RC.same(dev, want, (chunk, "device"))
        if chunk < n:  # the recalls from the first cut on: a call of their own under first_id + chunk, in one launch
            with RC.read_chunk(None):
                RC.same(call(RECALLS[chunk:], worlds[chunk:], FIRST_ID + chunk), RC.tail(want, chunk), (chunk, "ids"))
                if chunk == 1:
                    assert call(RECALLS[chunk:], worlds[chunk:], FIRST_ID)["holes"].tobytes() != want["holes"][chunk:].tobytes()
    at = NAMES.index("river")
    with RC.read_chunk(1):
        RC.same(call(RECALLS[at], worlds[at: at + 1], FIRST_ID + at), {k: v[at: at + 1] for k, v in want.items()}, "one recall")
    # worlds, world_out, attempts and status left out, in launches of 3: the drawn worlds' holes
    lib, packed, holes = _lib.load(), Recall.pack(RECALLS), np.zeros((n, deals), np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    with RC.read_chunk(3):
        assert lib.rp_nlhe_restrict(s._h, n, p(packed), deals, None, SEED, FIRST_ID, p(holes), None, None, None) == _lib.RP_OK
        RC.same(call(RECALLS, None, FIRST_ID), drawn, "drawn worlds, host")
        RC.same(from_device(s, s.restrict_device(rec, deals, None, SEED, FIRST_ID)), drawn, "drawn worlds, device")
    assert holes.tobytes() == drawn["holes"].tobytes() and holes.tobytes() != want["holes"].tobytes()

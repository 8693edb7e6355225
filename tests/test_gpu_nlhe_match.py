"""Matches on the device: rp_nlhe_match, host and _device forms, against the naive table of tests/nlhe_match_model.py (pinned by
tests/test_nlhe_match_model.py, which also asserts that the batches of tests/nlhe_match_cases.py hold every case named there).
Bit patterns and integers only: there is no tolerance.

Two 2^10-slot tables holding the rows the model's hands asked for (seat 0 reads the first, seat 1 the second), batches of at most 257
hands."""
import ctypes as C

import numpy as np
import pytest
import torch

import nlhe_aivat_model as AM
import nlhe_match_cases as K
import nlhe_match_model as MM
import nlhe_read_chunk as RC
from robopoker_amd import _lib
from robopoker_amd.nlhe import AIVAT_DTYPE, AivatHand, NlheSolver

pytestmark = pytest.mark.gpu

COLUMNS = (("won", np.int16), ("rejected", np.uint8), ("status", np.uint8))


def solvers(rows=None):
    """rows: load the first `rows` infosets only (room for a training step in the 1 024 slots)"""
    out = []
    for table in K.model().tables:
        s = NlheSolver(cap_log2=K.CAP_LOG2, batch=1, seed=1)
        s.load(*(x[:rows] for x in table), epoch=3)
        out.append(s)
    return out


@pytest.fixture(scope="module")
def pair(gpu):
    return solvers()


def as_map(past, present, choices, enc):
    return {(int(p), int(q), int(c)): enc[i].tobytes() for i, (p, q, c) in enumerate(zip(past, present, choices))}


def check(got, name, where=slice(None)):
    m = K.model()
    want = m.records(name)[where]
    assert got["hands"].dtype == AIVAT_DTYPE and got["hands"].tobytes() == want.tobytes(), \
        (name, [i for i in range(want.size) if got["hands"][i].tobytes() != want[i].tobytes()][:5])
    for f, dtype in COLUMNS:
        assert got[f].dtype == dtype and np.array_equal(got[f], m.column(name, f, dtype)[where]), (name, f)


def run(pair, name, device=False):
    _, n, args, one = K.CONFIGS[K.NAMES.index(name)]
    s0, s1 = pair
    if not device:
        return s0.match(n, None if one else s1, **args.kwargs())
    dev = s0.match_device(n, None if one else s1, **args.kwargs())
    s0.sync()
    assert all(t.is_cuda for t in dev.values())
    out = {k: v.cpu().numpy() for k, v in dev.items()}
    out["hands"] = out["hands"].reshape(-1).view(AIVAT_DTYPE)
    return out


@pytest.mark.parametrize("name", K.NAMES)
def test_host_form_equals_the_model(pair, name):
    got = run(pair, name)
    check(got, name)
    kinds, n_plays = got["hands"]["kind"], got["hands"]["n_plays"]
    assert all(not kinds[i, n_plays[i]:].any() and not got["hands"]["chips"][i, n_plays[i]:].any() for i in range(kinds.shape[0]))


def test_device_form_equals_the_host_form_and_the_second_table_matters(pair):
    m = K.model()
    for name in ("main", "main snap", "long street", "dirac fish snap 0 mirror 1"):
        check(run(pair, name, device=True), name)
    two, one = run(pair, "main", device=True), run(pair, "main one table", device=True)
    check(one, "main one table")
    differ = [a != b for a, b in zip(m.want["main"], m.want["main one table"])]
    assert [x.tobytes() != y.tobytes() for x, y in zip(two["hands"], one["hands"])] == differ and 0 < sum(differ) < len(differ)
    # h1 == h0 is h1 == NULL
    s0 = pair[0]
    _, n, args, _ = K.CONFIGS[K.NAMES.index("main one table")]
    assert s0.match(n, s0, **args.kwargs())["hands"].tobytes() == one["hands"].tobytes()


def test_a_hand_does_not_depend_on_the_batch_around_it(pair):
    m = K.model()
    s0, s1 = pair
    _, _, args, _ = K.CONFIGS[K.NAMES.index("main")]
    kw = dict(args.kwargs(), first_id=args.first_id - 96)
    whole = s0.match(257, s1, **kw)  # two workgroups of 256 lanes, the second with one hand
    assert not whole["status"].any() and whole["hands"][96:161].tobytes() == m.records("main").tobytes()
    for at, n in ((0, 1), (96, 1), (31, 65), (191, 65), (256, 1)):
        part = s0.match(n, s1, **dict(kw, first_id=kw["first_id"] + at))
        for f in ("hands", "won", "rejected", "status"):
            assert part[f].tobytes() == whole[f][at: at + n].tobytes(), (at, n, f)
    # an odd first id with mirror: hand 0 is the second of a pair whose first is not in the batch, hands 1 and 2 are a pair
    h = whole["hands"]
    assert kw["first_id"] % 2 == 1 and tuple(h[1]["hole"]) == tuple(h[2]["hole"][::-1]) and tuple(h[0]["hole"]) != tuple(h[1]["hole"][::-1])
    even = s0.match(4, s1, **dict(kw, first_id=kw["first_id"] - 1))
    assert tuple(even["hands"][0]["hole"]) == tuple(h[0]["hole"][::-1]) and even["hands"][1:].tobytes() == h[:3].tobytes()
    assert tuple(even["hands"][0]["draws"][:1]) == tuple(h[0]["draws"][:1]) or 0 in (even["hands"][0]["draws"][0], h[0]["draws"][0])


def test_a_queried_pair_steps_like_a_twin_never_queried(gpu):
    pair, twins = solvers(rows=32), solvers(rows=32)
    before = [(s.export(), s.epoch, s.counters()) for s in pair]
    _, n, args, _ = K.CONFIGS[K.NAMES.index("main")]
    pair[0].match(n, pair[1], **args.kwargs())
    pair[0].match_device(n, pair[1], **args.kwargs())
    pair[0].sync()
    after = [(s.export(), s.epoch, s.counters()) for s in pair]
    for b, a in zip(before, after):
        assert all(np.array_equal(x, y) for x, y in zip(b[0][:3], a[0][:3])) and b[0][3].tobytes() == a[0][3].tobytes()
        assert b[1:] == a[1:] == (3, (0, 0, 32))
    for s, t in zip(pair, twins):
        s.step()
        t.step()
        am, bm = as_map(*s.export()), as_map(*t.export())
        assert am.keys() == bm.keys() and len(am) > 32 and all(am[k] == bm[k] for k in am)
        assert (s.epoch, s.counters()) == (t.epoch, t.counters()) and s.epoch == 4


def test_the_records_go_to_aivat_without_a_host_copy(pair):
    s0, s1 = pair
    m = K.model()
    _, n, args, _ = K.CONFIGS[K.NAMES.index("pipeline")]
    assert (args.dealer, args.stacks, args.board_mode, n) == (0, (0, 0), 1, 65)
    dev = s0.match_device(n, s1, **args.kwargs())
    out = s0.aivat_device(dev["hands"])  # the tensor as it is
    s0.sync()
    assert not dev["status"].cpu().numpy().any() and not out["status"].cpu().numpy().any()
    want = m.want["pipeline"]
    past, present, choices, enc = m.tables[0]  # the evaluator reads the handle's own table at the nodes of both seats
    rows = {(int(p), int(q), int(c)): (enc["weight"][i], enc["payoff"][i]) for i, (p, q, c) in enumerate(zip(past, present, choices))}
    nodes = 0
    for i, w in enumerate(want):
        hand = AivatHand(w["holes"], w["draws"], w["plays"], seat=w["seat"], stacks=w["stacks"], dealer=w["dealer"], board_mode=w["board_mode"])
        ref = AM.corrections(hand, rows)
        assert ref[0] == AM.OK
        for k, f in enumerate(("hero", "villain", "chance", "total")):
            assert out[f][i].cpu().numpy().view(np.uint32) == np.float32(ref[1 + k]).view(np.uint32), (i, f)
        assert (int(out["n_action"][i]), int(out["n_chance"][i])) == ref[5:]
        nodes += ref[5] + ref[6]
    assert nodes > 65 and out["total"].cpu().numpy().any()
    won = dev["won"].cpu().numpy()
    assert np.array_equal(won, np.array([w["won"] for w in want], np.int16))
    adjusted = won.astype(np.float32) + out["total"].cpu().numpy()
    got, ref = NlheSolver.aivat_summarize(adjusted, 6.5), AM.summarize(adjusted, 6.5)
    assert all(np.float32(got[k]).view(np.uint32) == np.float32(ref[k]).view(np.uint32) for k in ref)
    got, ref = NlheSolver.match_summary(won), MM.summarize(won)
    assert got["hands"] == 65 and all(np.float64(got[k]).view(np.uint64) == np.float64(ref[k]).view(np.uint64) for k in ref if k != "hands")


def test_arguments(gpu):
    lib = _lib.load()
    s = NlheSolver(cap_log2=K.CAP_LOG2, batch=4, seed=2)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    hands, won, rej, st = np.zeros(2, AIVAT_DTYPE), np.zeros(2, np.int16), np.zeros(2, np.uint8), np.zeros(2, np.uint8)
    good = NlheSolver._match_args(seed=3)
    for fn in (lib.rp_nlhe_match, lib.rp_nlhe_match_device):
        assert fn(s._h, None, 0, C.byref(good), None, None, None, None) == _lib.RP_OK  # n = 0: no launch, whatever the pointers
        assert fn(None, None, 0, C.byref(good), None, None, None, None) == _lib.RP_ERR_INVALID
        assert fn(s._h, None, 0, None, None, None, None, None) == _lib.RP_ERR_INVALID
    # every output may be NULL, alone or together
    assert lib.rp_nlhe_match(s._h, None, 2, C.byref(good), None, None, None, None) == _lib.RP_OK
    assert lib.rp_nlhe_match(s._h, None, 2, C.byref(good), p(hands), p(won), p(rej), p(st)) == _lib.RP_OK
    only = np.zeros(2, np.int16)
    assert lib.rp_nlhe_match(s._h, None, 2, C.byref(good), None, p(only), None, None) == _lib.RP_OK and np.array_equal(only, won)
    assert not st.any() and hands["n_plays"].all()  # an empty table: every row absent, every policy uniform
    bad = [dict(agents=(3, 0)), dict(agents=(0, 3)), dict(dealer=3), dict(hero=2), dict(stacks=(0, 5)), dict(stacks=(-1, 5)), dict(stacks=(5, 0)),
           dict(mirror=2), dict(snap=2), dict(board_mode=2)]
    for kw in bad:
        assert lib.rp_nlhe_match(s._h, None, 2, C.byref(NlheSolver._match_args(**kw)), p(hands), p(won), p(rej), p(st)) == _lib.RP_ERR_INVALID, kw
        assert b"rp_nlhe_match" in lib.rp_last_error()
    for k in range(5):
        a = NlheSolver._match_args()
        a.reserved[k] = 1
        assert lib.rp_nlhe_match(s._h, None, 2, C.byref(a), p(hands), p(won), p(rej), p(st)) == _lib.RP_ERR_INVALID
    s.step()
    assert s.epoch == 1 and s.counters()[2] > 0


def hash_buckets(obs, street):
    """the hash encoder's bucket index of canonical observations (nl_bucket, encoder 0) for a whole isomorphism list"""
    m = np.uint64
    z = obs.astype(np.int64).view(np.uint64) ^ m((0x51ED270B5 * (street + 1)) & MM.RO.M64)
    z ^= z >> m(30)
    z *= m(0xBF58476D1CE4E5B9)
    z ^= z >> m(27)
    z *= m(0x94D049BB133111EB)
    z ^= z >> m(31)
    return (z % m((169, 256, 256, 101)[street])).astype(np.uint8)


def test_lookup_table_encoders(gpu):
    # the encoder over rp_lookup tables holding the hash encoder's buckets: every hole before the flop, the isomorphisms of the first 16
    # pockets after it.  A hand that ends before the flop answers as on the hash encoder; one that asks for a bucket the tables do not
    # hold is RP_RECALL_LOOKUP with zero outputs.  Two handles play only on one set of tables.
    from robopoker_amd import deuce

    def tables():
        out = []
        for street, (name, pockets) in enumerate((("pref", 1326), ("flop", 16), ("turn", 16), ("rive", 16))):
            obs = deuce.isomorphisms(name, 0, pockets)
            out.append(deuce.Lookup(name, obs, torch.from_numpy(hash_buckets(obs.cpu().numpy(), street)).to("cuda")))
        return out

    lib, m = _lib.load(), K.model()
    ta, tb = tables(), tables()
    a0, a1, b = (NlheSolver(cap_log2=K.CAP_LOG2, batch=1, seed=1, tables=t) for t in (ta, ta, tb))
    a0.load(*m.tables[0], epoch=3)
    a1.load(*m.tables[1], epoch=3)
    hashed = solvers()
    _, n, args, _ = K.CONFIGS[K.NAMES.index("main")]
    got = a0.match(n, a1, **args.kwargs())
    want = m.want["main"]
    preflop = np.array([w["draws"] == (0, 0, 0) for w in want])
    assert set(got["status"][~preflop]) <= {MM.OK, MM.LOOKUP} and (got["status"][~preflop] == MM.LOOKUP).any() and preflop.any()
    assert not got["status"][preflop].any() and got["hands"][preflop].tobytes() == m.records("main")[preflop].tobytes()
    assert np.array_equal(got["won"][preflop], m.column("main", "won", np.int16)[preflop])
    refused = got["status"] == MM.LOOKUP
    assert not got["hands"][refused].view(np.uint8).any() and not got["won"][refused].any() and not got["rejected"][refused].any()
    good = NlheSolver._match_args(seed=3)
    for h0, h1 in ((a0, hashed[0]), (hashed[0], a0), (a0, b)):
        assert lib.rp_nlhe_match(h0._h, h1._h, 2, C.byref(good), None, None, None, None) == _lib.RP_ERR_INVALID
        assert b"rp_nlhe_match" in lib.rp_last_error() and b"encoder" in lib.rp_last_error()
    for s in (a0, a1, b):
        s.close()
    for t in ta + tb:
        t.close()


def test_the_hands_do_not_depend_on_the_launch_chunk(pair):
    """RP_NLHE_READ_CHUNK (tests/nlhe_read_chunk.py) cuts the 65 hands of "main" into launches of 1, 3, 64 and 65: every launch counts
    its hand ids on from first_id.  The first id is odd and the hands are mirrored, so the pairs are the hands (1, 2), (3, 4), ...:
    launches of 3 keep (3, 4) together and part (5, 6)"""
    s0, s1 = pair
    _, n, args, one = K.CONFIGS[K.NAMES.index("main")]
    assert n % 16 and args.first_id % 2 == 1 and args.mirror and not one
    fields = ("hands", "won", "rejected", "status")

    def device(count, **kw):
        dev = s0.match_device(count, s1, **kw)
        s0.sync()
        out = {k: v.cpu().numpy() for k, v in dev.items()}
        return dict(out, hands=out["hands"].reshape(-1).view(AIVAT_DTYPE))

    with RC.read_chunk(None):
        want = s0.match(n, s1, **args.kwargs())
    check(want, "main")
    assert want["rejected"].any() and tuple(want["hands"][5]["hole"]) == tuple(want["hands"][6]["hole"][::-1])
    for chunk in RC.cuts(n):
        with RC.read_chunk(chunk):
            host, dev = s0.match(n, s1, **args.kwargs()), device(n, **args.kwargs())
        RC.same(host, want, (chunk, "host"))
        RC.same(dev, want, (chunk, "device"))
        check(host, "main")  # the model itself, on every hand of every launch
        if chunk < n:  # the hands from the first cut on: a call of their own under first_id + chunk, in one launch
            with RC.read_chunk(None):
                alone = s0.match(n - chunk, s1, **dict(args.kwargs(), first_id=args.first_id + chunk))
                RC.same(alone, RC.tail(want, chunk), (chunk, "ids"))
                unshifted = s0.match(n - chunk, s1, **args.kwargs())
                assert unshifted["hands"].tobytes() != want["hands"][chunk:].tobytes()
    with RC.read_chunk(1):  # one hand: the one-byte arrays end off the staging arena's alignment
        RC.same(s0.match(1, s1, **dict(args.kwargs(), first_id=args.first_id + 6)), {k: want[k][6:7] for k in fields}, "one hand")
    # the short-stacked mirrored hands of an even first id, 17 of them, in launches of 3: pairs (2, 3), (8, 9), (14, 15) are parted
    name = "fish dirac snap 1 mirror 1"
    _, n17, args17, _ = K.CONFIGS[K.NAMES.index(name)]
    assert n17 == 17 and args17.first_id % 2 == 0 and args17.mirror
    with RC.read_chunk(3):
        check(s0.match(n17, s1, **args17.kwargs()), name)
        check(device(n17, **args17.kwargs()), name)
    # every output but one left out, in launches of 3
    lib, a = _lib.load(), NlheSolver._match_args(**args.kwargs())
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    won, hands = np.zeros(n, np.int16), np.zeros(n, AIVAT_DTYPE)
    with RC.read_chunk(3):
        assert lib.rp_nlhe_match(s0._h, s1._h, n, C.byref(a), None, p(won), None, None) == _lib.RP_OK
        assert lib.rp_nlhe_match(s0._h, s1._h, n, C.byref(a), p(hands), None, None, None) == _lib.RP_OK
        assert lib.rp_nlhe_match_device(s0._h, s1._h, n, C.byref(a), None, None, None, None) == _lib.RP_OK
        s0.sync()
    RC.same((won, hands), (want["won"], want["hands"]), "one output alone")

"""Search matches on the device: rp_nlhe_search_match, host and _device forms, against the naive composition of
tests/nlhe_search_model.py (pinned by tests/test_nlhe_search_model.py, which also asserts that the batches of tests/nlhe_search_cases.py
hold every case named there) and, step by step, against the library's own rp_nlhe_belief + rp_nlhe_subgame_solve.  Bit patterns and
integers only: there is no tolerance.

Two tables holding the rows the model's hands and solves asked for (seat 0 reads the first, seat 1 the second); batches of 9 hands,
except where a wavefront and a workgroup of the advance kernel are crossed (65, 257)."""
import numpy as np
import pytest
import torch

import nlhe_search_cases as SC
import nlhe_search_model as XM
from robopoker_amd.nlhe import AIVAT_DTYPE, FRONTIER_DTYPE, SEARCH_STEP_DTYPE, NlheSolver

pytestmark = pytest.mark.gpu

COLUMNS = (("won", np.int16), ("rejected", np.uint8), ("status", np.uint8), ("searched", np.uint8), ("unsolved", np.uint8))
FIELDS = ("hands",) + tuple(f for f, _ in COLUMNS) + ("steps",)


def solvers():
    m, out = SC.model(), []
    for table in m.tables:
        s = NlheSolver(cap_log2=m.cap_log2, batch=1, seed=1)
        s.load(*table, epoch=SC.EPOCH)
        out.append(s)
    return out


@pytest.fixture(scope="module")
def pair(gpu):
    return solvers()


def kwargs(name, **over):
    _, n, args, sargs, one = SC.config(name)
    return n, one, dict(dict(args.kwargs(), **sargs.kwargs()), **over)


def run(pair, name, device=False, n=None, **over):
    n0, one, kw = kwargs(name, **over)
    n = n0 if n is None else n
    s0, s1 = pair
    if not device:
        return s0.search_match(n, None if one else s1, **kw)
    dev = s0.search_match_device(n, None if one else s1, **kw)  # returns when the match is finished
    assert all(t.is_cuda for t in dev.values())
    out = {k: v.cpu().numpy() for k, v in dev.items()}
    out["hands"] = out["hands"].reshape(-1).view(AIVAT_DTYPE)
    out["steps"] = out["steps"].reshape(-1).view(SEARCH_STEP_DTYPE).reshape(n, -1)
    return out


def check(got, name):
    m = SC.model()
    want = m.records(name)
    assert got["hands"].dtype == AIVAT_DTYPE and got["hands"].tobytes() == want.tobytes(), \
        (name, [i for i in range(want.size) if got["hands"][i].tobytes() != want[i].tobytes()][:5])
    for f, dtype in COLUMNS:
        assert got[f].dtype == dtype and np.array_equal(got[f], m.column(name, f, dtype)), (name, f, got[f], m.column(name, f, dtype))
    steps = m.steps(name)
    assert got["steps"].dtype == SEARCH_STEP_DTYPE and got["steps"].shape == steps.shape
    for i in range(steps.shape[0]):
        for k in range(steps.shape[1]):
            if got["steps"][i, k].tobytes() != steps[i, k].tobytes():
                a, b = got["steps"][i, k], steps[i, k]
                bad = [f for f in SEARCH_STEP_DTYPE.names if a[f].tobytes() != b[f].tobytes()]
                raise AssertionError((name, i, k, bad, [(a[f], b[f]) for f in bad if f not in ("recall", "result")],
                                      [(f, a["result"][f], b["result"][f]) for f in a["result"].dtype.names
                                       if "result" in bad and a["result"][f].tobytes() != b["result"][f].tobytes()]))


def same(a, b, fields=FIELDS):
    for f in fields:
        assert a[f].tobytes() == b[f].tobytes(), f


def test_no_search_seat_is_rp_nlhe_match_byte_for_byte(pair):
    s0, s1 = pair
    _, _, kw = kwargs("world blueprint", search=("none", "none"), stacks=(0, 0))
    match_kw = {k: kw[k] for k in ("seed", "first_id", "stacks", "agents", "dealer", "hero", "mirror", "snap", "board_mode")}
    for n in (65, 257):  # a wavefront and a workgroup of the advance kernel are crossed
        got, want = s0.search_match(n, s1, **kw), s0.match(n, s1, **match_kw)
        same(got, want, ("hands", "won", "rejected", "status"))
        assert not got["searched"].any() and not got["unsolved"].any() and not got["steps"].view(np.uint8).any()
        assert want["hands"]["n_plays"].all() and len(set(want["hands"]["draws"][:, 0])) > 8


@pytest.mark.parametrize("name", SC.NAMES)
def test_host_form_equals_the_model(pair, name):
    check(run(pair, name), name)


def test_device_form_equals_the_host_form(pair):
    for name in ("world fish", "both one table"):
        check(run(pair, name, device=True), name)


def entry_of(recall):
    """INTEGRATION.md's adapt_full entry of a recall: holes[pov] only, the prefix = the trailing choice edges, first 12"""
    e = np.zeros(1, FRONTIER_DTYPE)
    pov, n = int(recall["pov"]), int(recall["n_edges"])
    e["holes"][0, pov] = recall["hole"]
    for f in ("draws", "stacks", "dealer", "n_edges", "edges"):
        e[f][0] = recall[f]
    e["internal"] = pov
    edges = [int(x) for x in recall["edges"][:n]]
    tail = edges[len(edges) - edges[::-1].index(1):] if 1 in edges else edges
    tail = tail[:12]
    e["n_prefix"], e["prefix"][0, : len(tail)] = len(tail), tail
    return e


@pytest.mark.parametrize("name", SC.NAMES)
def test_every_traced_step_is_what_the_two_public_calls_answer(pair, name):
    _, _, args, sargs, one = SC.config(name)
    got = run(pair, name)
    asked = 0
    for i in range(got["steps"].shape[0]):
        for k in range(min(int(got["searched"][i]), SC.STEPS_CAP)):
            st = got["steps"][i, k]
            assert st["fallback"] not in (XM.LENGTH, XM.CAP) and st["solve_id"] == (args.first_id + i) * 256 + st["decision"]
            s = pair[0] if one or st["seat"] == 0 else pair[1]  # a seat's solves run against its own handle's table
            rec = st["recall"].reshape(1)
            bel = s.belief(rec)
            entry = entry_of(rec[0])
            street = sum(1 for d in rec[0]["draws"] if d)
            res, _, _ = s.subgame_solve(entry, bel, street - 1 if sargs.origin_mode else None, sargs.iterations, sargs.rollouts, sargs.bias,
                                        sargs.prior, sargs.search_seed, int(st["solve_id"]))
            assert int(bel["status"][0]) == int(st["belief_status"]) and res[0].tobytes() == st["result"].tobytes(), (name, i, k)
            asked += 1
        assert not got["steps"][i, int(got["searched"][i]):].view(np.uint8).any()
    assert asked == sum(min(len(w["steps"]), SC.STEPS_CAP) for w in SC.model().want[name]) and asked > 0


def test_a_hand_does_not_depend_on_the_batch_around_it(pair):
    s0, s1 = pair
    n, _, kw = kwargs("both")
    whole = run(pair, "both")
    for i in range(n):  # hand by hand
        part = s0.search_match(1, s1, **dict(kw, first_id=kw["first_id"] + i))
        for f in FIELDS:
            assert part[f].tobytes() == whole[f][i: i + 1].tobytes(), (i, f)
    # 65 hands — more than a wavefront of parked hands are compacted — split in two calls
    big = s0.search_match(65, s1, **dict(kw, first_id=kw["first_id"] - 20))
    same({f: big[f][20:29] for f in FIELDS}, whole)
    assert int(big["searched"].astype(np.int64).sum()) > int(whole["searched"].astype(np.int64).sum())
    for at, m in ((0, 31), (31, 34)):
        part = s0.search_match(m, s1, **dict(kw, first_id=kw["first_id"] - 20 + at))
        same(part, {f: big[f][at: at + m] for f in FIELDS})


def test_two_tables_and_one_table_differ_where_the_model_says(pair):
    m = SC.model()
    two, one = run(pair, "both", device=True), run(pair, "both one table", device=True)
    differ = [a["plays"] != b["plays"] or a["won"] != b["won"] for a, b in zip(m.want["both"], m.want["both one table"])]
    assert [x.tobytes() != y.tobytes() for x, y in zip(two["hands"], one["hands"])] == differ and 0 < sum(differ) < len(differ)
    s0 = pair[0]
    n, _, kw = kwargs("both one table")
    assert s0.search_match(n, s0, **kw)["steps"].tobytes() == one["steps"].tobytes()  # h1 == h0 is h1 == NULL


def test_origin_mode_1_plays_rollouts(pair):
    got = run(pair, "origin")
    solved = got["steps"][got["steps"]["result"]["iterations"] > 0]
    river = solved["recall"]["draws"][:, 2] != 0  # no street lies beyond the river: no frontier there
    assert river.any() and not river.all() and not solved["result"]["rollouts"][river].any()
    assert (solved["result"]["rollouts"][~river] > 0).all() and (solved["result"]["frontiers"][~river] > 0).all()
    none = run(pair, "origin", origin_mode=0)
    assert not none["steps"]["result"]["rollouts"].any() and none["steps"]["result"]["iterations"].any()


def test_both_tables_are_read_only(pair):
    before = [(s.export(), s.epoch, s.counters()) for s in pair]
    run(pair, "both")
    run(pair, "world fish", device=True)
    after = [(s.export(), s.epoch, s.counters()) for s in pair]
    for b, a in zip(before, after):
        assert all(np.array_equal(x, y) for x, y in zip(b[0][:3], a[0][:3])) and b[0][3].tobytes() == a[0][3].tobytes()
        assert b[1:] == a[1:] and a[1] == SC.EPOCH


def test_the_records_go_to_aivat_without_a_host_copy(pair):
    s0, s1 = pair
    n, _, kw = kwargs("world blueprint")
    dev = s0.search_match_device(n, s1, **kw)
    out = s0.aivat_device(dev["hands"])  # the tensor as it is
    s0.sync()
    host = s0.aivat(dev["hands"].cpu().numpy().reshape(-1).view(AIVAT_DTYPE))
    assert not dev["status"].cpu().numpy().any() and dev["searched"].cpu().numpy().any()
    for f in ("hero", "villain", "chance", "total", "n_action", "n_chance", "status"):
        assert out[f].cpu().numpy().tobytes() == np.ascontiguousarray(host[f]).tobytes(), f
    assert out["total"].cpu().numpy().any() and isinstance(dev["hands"], torch.Tensor)


REFUSED_IDS = (326, 437, 637, 1910, 2075, 3895, 4021)  # found by search with the model; the test asserts what the search was for


def test_a_hand_refused_after_a_search_decision_takes_its_steps_back(gpu, monkeypatch):
    # The only way a hand of these fixtures ends without outputs after it has traced a step: encoders over rp_lookup tables that hold
    # every hole before the flop and the isomorphisms of the first 16 pockets after it (tests/test_gpu_nlhe_match.py).  Seat 0 searches
    # with a hole the tables know, traces its decision — the belief is refused, RP_RECALL_LOOKUP, because the tables do not know the
    # opponent's candidates, so the step is fallback 1 and plays the blueprint — and then seat 1 asks for a bucket the tables do not
    # hold: the hand is RP_RECALL_LOOKUP, and its steps, searched and unsolved are taken back.  The model is the search model with the
    # tables' buckets and that refused belief; no solve of it is compared.
    import nlhe_match_cases as K
    import nlhe_match_model as MM
    import nlhe_range_model as RM
    import oracle_deuce as OD
    from robopoker_amd import deuce
    from test_gpu_nlhe_match import hash_buckets

    tables, known = [], []
    for street, (name, pockets) in enumerate((("pref", 1326), ("flop", 16), ("turn", 16), ("rive", 16))):
        obs = deuce.isomorphisms(name, 0, pockets)
        host = obs.cpu().numpy()
        known.append(np.sort(host))
        tables.append(deuce.Lookup(name, obs, torch.from_numpy(hash_buckets(host, street)).to("cuda")))

    def bucket(street, hole, board):
        o = OD.obs_i64(*OD.isomorphism(hole, board))
        k = int(np.searchsorted(known[street], o))
        return RM._bucket(street, hole, board) if k < known[street].size and known[street][k] == o else None

    asked = {}

    def no_belief(sargs, hand_id, decision, turn, witness, stacks, dealer, dealt, hole, rows, bp_epoch, key, slots, bp):
        asked[hand_id] = asked.get(hand_id, 0) + 1
        return dict(solve_id=hand_id * 256 + decision, recall=None, result=None, belief_status=MM.LOOKUP, bp=list(bp), p=list(bp), seat=turn,
                    decision=decision, fallback=XM.BELIEF)

    monkeypatch.setattr(XM, "search_decision", no_belief)
    args = MM.Args(seed=SC.SEED, stacks=SC.SHORT, dealer=2, snap=True)
    sargs = XM.SearchArgs(search=("world", "none"), iterations=2, rollouts=1, visit_threshold=2, steps_cap=SC.STEPS_CAP, search_seed=SC.SEARCH_SEED)
    rows = (SC.Rows(1), SC.Rows(2))  # fresh: the tables hold what these hands ask for
    want = [XM.play(i, args, sargs, rows, SC.EPOCH, bucket=bucket) for i in REFUSED_IDS]
    taken_back = [w["status"] == MM.LOOKUP and asked.get(i, 0) > 0 for i, w in zip(REFUSED_IDS, want)]
    assert sum(taken_back) >= 3 and any(w["status"] == MM.LOOKUP and i not in asked for i, w in zip(REFUSED_IDS, want))
    assert any(w["status"] == MM.OK and w["searched"] == w["unsolved"] > 0 for w in want) and any(w["status"] == MM.OK and not w["searched"] for w in want)
    loaded = [r.table() for r in rows]
    pair = [NlheSolver(cap_log2=max(8, max((2 * t[0].size).bit_length() for t in loaded)), batch=1, seed=1, tables=tables) for _ in loaded]
    for s, t in zip(pair, loaded):
        s.load(*t, epoch=SC.EPOCH)
    kw = dict(args.kwargs(), **sargs.kwargs())
    for i, w, back in zip(REFUSED_IDS, want, taken_back):
        for form in (False, True):
            if form:
                dev = pair[0].search_match_device(1, pair[1], **dict(kw, first_id=i))
                got = {k: v.cpu().numpy() for k, v in dev.items()}
                got["hands"], got["steps"] = got["hands"].reshape(-1).view(AIVAT_DTYPE), got["steps"].reshape(-1).view(SEARCH_STEP_DTYPE).reshape(1, -1)
            else:
                got = pair[0].search_match(1, pair[1], **dict(kw, first_id=i))
            assert got["hands"].tobytes() == K.pack([w]).tobytes(), i
            for f, dtype in COLUMNS:
                assert got[f][0] == dtype(w[f]), (i, f, got[f], w[f])
            steps = got["steps"][0]
            if back or w["status"] != MM.OK:
                assert not steps.view(np.uint8).any() and not got["searched"][0] and not got["unsolved"][0], i
                continue
            assert len(w["steps"]) <= SC.STEPS_CAP and not steps[len(w["steps"]):].view(np.uint8).any()
            for k, st in enumerate(w["steps"]):  # the belief was refused: the step is a fallback to the blueprint's policy
                assert (steps[k]["solve_id"], steps[k]["decision"], steps[k]["seat"], steps[k]["edge"], steps[k]["fallback"]) == (
                    st["solve_id"], st["decision"], st["seat"], st["edge"], XM.BELIEF) and steps[k]["belief_status"] != MM.OK, (i, k)
                n = len(st["bp"])
                assert steps[k]["bp"][:n].tobytes() == np.array(st["bp"], np.float32).tobytes() and steps[k]["p"].tobytes() == steps[k]["bp"].tobytes()
    # A trace shorter than the uncapped one.  steps_cap = 1: a refused hand takes back exactly its one record and writes nothing past
    # it.  steps_cap = 0 with a trace address all the same: the hand has taken more search decisions than the cap (1 > 0), nothing of
    # the trace is touched, searched and unsolved are zeroed.  The _device form on a trace allocated for one hand more, pre-filled:
    # the extra row is untouched.  What stays unreached is the take-back's min(n_steps, steps_cap) with n_steps > steps_cap > 0: no
    # hand of 12 000 ids is refused after TWO search decisions of seat 0 — seat 1 is refused at its first turn in between.
    import ctypes as C
    import itertools

    from robopoker_amd import _lib
    from robopoker_amd.nlhe import _dptr

    d = torch.device("cuda", pair[0].device)
    for (i, w, back), cap in itertools.product(zip(REFUSED_IDS, want, taken_back), (1, 0)):
        a = NlheSolver._search_args(**dict(kw, first_id=i, steps_cap=cap))
        steps = torch.full((2, 1, SEARCH_STEP_DTYPE.itemsize), 0xA5, dtype=torch.uint8, device=d)
        counts = torch.full((2, 2), 0xA5, dtype=torch.uint8, device=d)  # searched, unsolved
        torch.cuda.current_stream(d).synchronize()
        _lib.check(_lib.load().rp_nlhe_search_match_device(pair[0]._h, pair[1]._h, 1, C.byref(a), None, None, None, None, _dptr(counts[0], 1),
                                                           _dptr(counts[1], 1), _dptr(steps, 1)))
        got, counts = steps.cpu().numpy(), counts.cpu().numpy()
        assert (got[1] == 0xA5).all() and (counts[:, 1] == 0xA5).all(), i
        first = got[0].reshape(-1).view(SEARCH_STEP_DTYPE)[0]
        if back or w["status"] != MM.OK:
            assert not counts[:, 0].any() and (not got[0].any() if cap else (got[0] == 0xA5).all()), (i, cap)
            continue
        assert tuple(counts[:, 0]) == (w["searched"], w["unsolved"]), i  # the uncapped counts
        if cap == 0:
            assert (got[0] == 0xA5).all(), i
            continue
        if not w["steps"]:
            assert not got[0].any(), i
            continue
        st = w["steps"][0]
        assert (first["solve_id"], first["decision"], first["seat"], first["edge"], first["fallback"]) == (
            st["solve_id"], st["decision"], st["seat"], st["edge"], XM.BELIEF) and first["belief_status"] != MM.OK, i
        assert first["bp"][: len(st["bp"])].tobytes() == np.array(st["bp"], np.float32).tobytes() and first["p"].tobytes() == first["bp"].tobytes()
    for s in pair:
        s.close()
    for t in tables:
        t.close()


def test_an_empty_batch_with_a_trace(pair):
    s0, s1 = pair
    _, _, kw = kwargs("world blueprint")
    host, dev = s0.search_match(0, s1, **kw), s0.search_match_device(0, s1, **kw)
    assert host["steps"].shape == (0, SC.STEPS_CAP) and tuple(dev["steps"].shape) == (0, SC.STEPS_CAP, SEARCH_STEP_DTYPE.itemsize)
    assert all(v.size == 0 for v in host.values()) and all(v.numel() == 0 for v in dev.values())

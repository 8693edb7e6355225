"""rp_nlhe_search_match at the sizes it was built for, and where its trace ends: a batch that fills a chunk of 1 024 hands and enters
a second (1 089 hands, both seats searching, several hundred solves of either seat in one round), the scratch a call inherits from the
call before, and a steps_cap below a hand's search decisions.  Bytes and integers only: there is no tolerance.

The thousand hands are compared against the replay model of tests/nlhe_search_replay.py — the model's own hand loop, the belief and
the harvest of every search decision asked of the library's two public calls — which is pinned here against the full CPU model on two
of the shared configs; the first nine hands of the big batch are "both"'s own and are compared against the full CPU model directly.

THE LIMIT THIS MODULE KEEPS on the MI355X: the big batch's fixture, which runs once, under 5 s; every test's own call under 0.5 s.
The issue's margin — five times the parent's test_host_form_equals_the_model, which takes under 5 ms per config — cannot hold a
thousand hands' model: the fixture's cost is the replay model's 1 883 solves and 16 beliefs through the public calls and its hands
replayed in Python round by round, not the library's two forms of the 1 089 hands.  Measured: fixture 2.3 s; the slowest call 0.07 s
(the three further calls of 1 089 hands of the stale-scratch test).  Under the host execution model (RP_EMUL=1) the fixture takes 9 to
18 s at the full 1 089 hands, so no reduced size is kept for it."""
import ctypes as C

import numpy as np
import pytest
import torch

import nlhe_match_cases as K
import nlhe_search_cases as SC
import nlhe_search_replay as RP
from robopoker_amd import _lib
from robopoker_amd.nlhe import AIVAT_DTYPE, SEARCH_STEP_DTYPE, NlheSolver, _dptr
from test_gpu_nlhe_search_match import COLUMNS, FIELDS, kwargs, run, same, solvers

pytestmark = pytest.mark.gpu

OUTPUTS = ("hands",) + tuple(f for f, _ in COLUMNS)  # everything but the trace


@pytest.fixture(scope="module")
def pair(gpu):
    return solvers()


def loaded(tables, cap_log2):
    out = []
    for t in tables:
        s = NlheSolver(cap_log2=cap_log2, batch=1, seed=1)
        s.load(*t, epoch=SC.EPOCH)
        out.append(s)
    return out


def host_view(dev, n):
    out = {k: v.cpu().numpy() for k, v in dev.items()}
    out["hands"] = out["hands"].reshape(-1).view(AIVAT_DTYPE)
    out["steps"] = out["steps"].reshape(-1).view(SEARCH_STEP_DTYPE).reshape(n, dev["steps"].shape[1])
    return out


def play(pair, name, device=False, **over):
    """test_gpu_nlhe_search_match.run, whose device form cannot shape an empty trace"""
    n, one, kw = kwargs(name, **over)
    s0, s1 = pair
    if not device:
        return s0.search_match(n, None if one else s1, **kw)
    return host_view(s0.search_match_device(n, None if one else s1, **kw), n)


def equals(got, hands, cap, what):
    """the library's outputs against a model's hands (nlhe_search_model.match's list), the trace cut at cap"""
    want = K.pack(hands)
    assert got["hands"].dtype == AIVAT_DTYPE and got["hands"].tobytes() == want.tobytes(), \
        (what, [i for i in range(want.size) if got["hands"][i].tobytes() != want[i].tobytes()][:5])
    for f, dtype in COLUMNS:
        col = np.array([w[f] for w in hands], dtype)
        assert got[f].dtype == dtype and np.array_equal(got[f], col), (what, f, np.flatnonzero(got[f] != col)[:5])
    steps = SC.pack_steps(hands, cap)
    assert got["steps"].dtype == SEARCH_STEP_DTYPE and got["steps"].shape == steps.shape, (what, got["steps"].shape)
    if got["steps"].tobytes() != steps.tobytes():
        bad = [(i, k) for i in range(steps.shape[0]) for k in range(steps.shape[1]) if got["steps"][i, k].tobytes() != steps[i, k].tobytes()]
        a, b = got["steps"][bad[0]], steps[bad[0]]
        raise AssertionError((what, len(bad), bad[:5], [f for f in SEARCH_STEP_DTYPE.names if a[f].tobytes() != b[f].tobytes()]))


class Big:
    """the big batch's handles, its replay model and its two forms, computed once"""

    def __init__(self):
        b = RP.big_batch()
        self.n, self.cap, self.args, self.sargs, self.tables, self.cap_log2 = RP.BIG_N, RP.BIG_CAP, b["args"], b["sargs"], b["tables"], b["cap_log2"]
        self.pair = loaded(self.tables, self.cap_log2)
        self.kw = dict(self.args.kwargs(), **self.sargs.kwargs())
        self.before = [(s.export(), s.epoch, s.counters()) for s in self.pair]
        self.replay = RP.Replay(self.pair, [RP.Table(t) for t in self.tables], self.args, self.sargs, SC.EPOCH)
        self.want = self.replay.match(self.n)
        self.host = self.call()
        self.dev = host_view(self.pair[0].search_match_device(self.n, self.pair[1], **self.kw), self.n)

    def call(self, n=None, pair=None, **over):
        s0, s1 = pair or self.pair
        return s0.search_match(self.n if n is None else n, s1, **dict(self.kw, **over))


@pytest.fixture(scope="module")
def big(gpu):
    return Big()


def test_the_replay_model_is_the_full_model_where_that_is_pinned(pair):
    m = SC.model()
    tables = [RP.Table(t) for t in m.tables]
    for name in ("both", "world fish"):
        _, n, args, sargs, one = SC.config(name)
        assert not one
        replay = RP.Replay(pair, tables, args, sargs, SC.EPOCH)
        got, want = replay.match(n), m.want[name]
        assert K.pack(got).tobytes() == m.records(name).tobytes(), name
        for f, dtype in COLUMNS:
            assert np.array_equal(np.array([w[f] for w in got], dtype), m.column(name, f, dtype)), (name, f)
        assert SC.pack_steps(got).tobytes() == m.steps(name).tobytes(), name
        assert [[s["fallback"] for s in w["steps"]] for w in got] == [[s["fallback"] for s in w["steps"]] for w in want]
        # the rounds are the hands' solves in order: as many requests as steps, a hand's k-th in round k
        assert sum(len(r) for r in replay.rounds) == sum(len(w["steps"]) for w in want) == len(replay.known)
        assert [sum(1 for r in replay.rounds for j, _ in r if j == i) for i in range(n)] == [len(w["steps"]) for w in want]


def test_the_big_batch_is_what_it_is_for(big):
    """asserted from the model, never from the library: the batch exercises what it was built to"""
    counts = big.replay.counts(0, RP.CHUNK)
    # every thread of k_nl_search_compact's scan holds a request, and seat 1's list starts beyond a wavefront of seat 0's
    assert counts[0] == RP.big_batch()["first"] and min(counts[0]) > 256, counts
    assert any(a > 64 and b > 64 for a, b in counts[1:]) and len(counts) > big.cap + 1, counts  # later rounds are no stubs
    second = big.replay.counts(RP.CHUNK, big.n)
    assert second[0][0] > 0 and second[0][1] > 0 and len(second) > big.cap, second
    most = max(len(w["steps"]) for w in big.want)
    assert most > big.cap and most <= SC.STEPS_CAP + 6  # hands go on untraced, parked and resumed, in the middle of a chunk
    assert sum(len(w["steps"]) > big.cap for w in big.want[: RP.CHUNK]) > 64 and any(len(w["steps"]) > big.cap for w in big.want[RP.CHUNK:])
    codes = {s["fallback"] for w in big.want for s in w["steps"]}
    assert RP.XM.SOLVED in codes and len(codes) > 1 and all(w["status"] == 0 for w in big.want)
    assert sum(len(w["steps"]) for w in big.want) > RP.CHUNK


def test_a_full_chunk_and_the_next_equal_the_models(big):
    equals(big.host, big.want, big.cap, "host form")
    equals(big.dev, big.want, big.cap, "device form")
    # hands [0, 9) are "both"'s: the full CPU model, independent of the replay model
    m, nine = SC.model(), {f: big.host[f][:9] for f in FIELDS}
    equals(nine, m.want["both"], big.cap, "the full model")
    assert nine["steps"].tobytes() == m.steps("both")[:, : big.cap].tobytes()


def test_the_second_chunk_on_its_own(big):
    at = RP.CHUNK
    part = big.call(big.n - at, first_id=big.args.first_id + at)
    same(part, {f: big.host[f][at:] for f in FIELDS})


def test_a_chunk_of_1024_and_one_of_1025(big):
    for n in (RP.CHUNK, RP.CHUNK + 1):
        same(big.call(n), {f: big.host[f][:n] for f in OUTPUTS}, OUTPUTS)


def test_a_call_does_not_read_the_scratch_of_the_call_before(big):
    # a stale NsHand.done / parked / place, or a stale dense list, is what the first round of the third call would read
    over = dict(first_id=big.args.first_id + 5000, search=("world", "none"), steps_cap=SC.STEPS_CAP)
    between = big.call(9, **over)
    again = big.call()
    same(again, big.host)
    fresh = loaded(big.tables, big.cap_log2)
    same(between, big.call(9, pair=fresh, **over))
    assert between["searched"].any() and not (between["steps"]["seat"] != 0).any()
    for s in fresh:
        s.close()


def test_both_tables_stay_read_only_across_the_big_batch(big):
    after = [(s.export(), s.epoch, s.counters()) for s in big.pair]
    for b, a in zip(big.before, after):
        assert all(np.array_equal(x, y) for x, y in zip(b[0][:3], a[0][:3])) and b[0][3].tobytes() == a[0][3].tobytes()
        assert b[1:] == a[1:] and a[1] == SC.EPOCH


# ---- the trace cap


@pytest.mark.parametrize("name", ("both", "deep"))
def test_a_trace_shorter_than_the_hands(pair, name):
    m = SC.model()
    hands = m.want[name]
    most = max(len(w["steps"]) for w in hands)
    assert 3 <= most <= SC.STEPS_CAP
    whole = run(pair, name)
    for cap in (1, most - 1):
        for device in (False, True):
            got = run(pair, name, device=device, steps_cap=cap)
            equals(got, hands, cap, (name, cap, device))  # searched and unsolved are the uncapped counts
            same(got, whole, OUTPUTS)
            assert got["steps"].tobytes() == whole["steps"][:, :cap].tobytes()
        assert any(w["searched"] > cap for w in hands)


def test_no_trace_at_all(pair):
    # steps_cap = 0 is steps = NULL through the ABI: NlheSolver.search_match passes no address then
    for name in ("both", "deep"):
        whole = run(pair, name)
        for device in (False, True):
            got = play(pair, name, device=device, steps_cap=0)
            assert got["steps"].shape == (whole["hands"].size, 0)
            same(got, whole, OUTPUTS)
    # ... and the _device form with a NULL steps and a steps_cap the args still state is refused before anything runs
    n, _, kw = kwargs("both")
    a = NlheSolver._search_args(**kw)
    assert a.steps_cap == SC.STEPS_CAP
    lib = _lib.load()
    assert lib.rp_nlhe_search_match_device(pair[0]._h, pair[1]._h, n, C.byref(a), *[None] * 7) == _lib.RP_ERR_INVALID
    a.steps_cap = 0  # every output NULL: the match is played and nothing is written
    assert lib.rp_nlhe_search_match_device(pair[0]._h, pair[1]._h, n, C.byref(a), *[None] * 7) == _lib.RP_OK
    assert lib.rp_nlhe_search_match(pair[0]._h, pair[1]._h, n, C.byref(a), *[None] * 7) == _lib.RP_OK


def test_the_trace_ends_where_the_next_hand_begins(pair):
    """a trace of n hands in an allocation of n + 1, pre-filled: nothing is written past a hand's steps_cap records, and a capped
    hand's last record is not the next hand's first"""
    n, _, kw = kwargs("both")
    hands = SC.model().want["both"]
    cap = 2
    a = NlheSolver._search_args(**dict(kw, steps_cap=cap))
    d = torch.device("cuda", pair[0].device)
    steps = torch.full((n + 1, cap, SEARCH_STEP_DTYPE.itemsize), 0xA5, dtype=torch.uint8, device=d)
    searched = torch.empty(n, dtype=torch.uint8, device=d)
    torch.cuda.current_stream(d).synchronize()
    _lib.check(_lib.load().rp_nlhe_search_match_device(pair[0]._h, pair[1]._h, n, C.byref(a), None, None, None, None, _dptr(searched, n), None,
                                                       _dptr(steps, n)))
    got = steps.cpu().numpy()
    assert (got[n] == 0xA5).all()
    assert got[:n].reshape(-1).view(SEARCH_STEP_DTYPE).reshape(n, cap).tobytes() == SC.pack_steps(hands, cap).tobytes()
    assert np.array_equal(searched.cpu().numpy(), [w["searched"] for w in hands]) and max(w["searched"] for w in hands) > cap


# ---- RP_SEARCH_FALLBACK_SOLVE


SOLVE_FIRST, SOLVE_N = 300, 65


def test_a_solve_refused_after_a_belief_that_was_not(gpu):
    """The one route to RP_SEARCH_FALLBACK_SOLVE found through the ABI: encoders over rp_lookup tables that hold every hole before the
    flop and on it, and the isomorphisms of the first 16 pockets beyond (tests/test_gpu_nlhe_match.py), with origin_mode 1.  A flop
    decision's belief is RP_RECALL_OK — every candidate hole has its flop bucket — while the rollouts of the solve's frontiers walk onto
    the turn and ask for buckets the tables do not hold: the solve is RP_RECALL_LOOKUP, the step carries the zeroed result with that
    status, plays the blueprint and counts in unsolved.  A hand that goes on to the turn is refused there and takes the step back; a hand
    that ends on the flop keeps it; where its tree has no frontier (a shove to call or fold) a later flop solve of the same hand is
    played.  No CPU model of the solver reads lookup tables, so the model is the replay model alone: its code for a step is
    nlhe_search_model's order over the statuses the two public calls answer."""
    import nlhe_match_model as MM
    import nlhe_range_model as RM
    import oracle_deuce as OD
    from robopoker_amd import deuce
    from test_gpu_nlhe_match import hash_buckets

    tables, known = [], []
    for street, (name, pockets) in enumerate((("pref", 1326), ("flop", 1326), ("turn", 16), ("rive", 16))):
        obs = deuce.isomorphisms(name, 0, pockets)
        host = obs.cpu().numpy()
        known.append(np.sort(host))
        tables.append(deuce.Lookup(name, obs, torch.from_numpy(hash_buckets(host, street)).to("cuda")))

    def bucket(street, hole, board):
        o = OD.obs_i64(*OD.isomorphism(hole, board))
        k = int(np.searchsorted(known[street], o))
        return RM._bucket(street, hole, board) if k < known[street].size and known[street][k] == o else None

    m = SC.model()
    args = MM.Args(seed=SC.SEED, first_id=SOLVE_FIRST, stacks=SC.SHORT, dealer=2, snap=True)
    sargs = RP.XM.SearchArgs(search=("world", "world"), origin_mode=1, iterations=2, rollouts=1, visit_threshold=2, steps_cap=SC.STEPS_CAP,
                             search_seed=SC.SEARCH_SEED)
    pair = [NlheSolver(cap_log2=m.cap_log2, batch=1, seed=1, tables=tables) for _ in m.tables]
    for s, t in zip(pair, m.tables):
        s.load(*t, epoch=SC.EPOCH)
    want = RP.Replay(pair, [RP.Table(t) for t in m.tables], args, sargs, SC.EPOCH, bucket).match(SOLVE_N)
    # asserted from the model: what the batch is for
    kept = [s for w in want if w["status"] == MM.OK for s in w["steps"]]
    refused = [s for s in kept if s["fallback"] == RP.XM.SOLVE]
    assert len(refused) >= 3 and all(s["belief_status"] == MM.OK and int(s["result"]["status"]) == MM.LOOKUP for s in refused)
    assert all(not s["result"]["refined"].any() and not s["result"]["visits"].any() and not s["result"]["iterations"] for s in refused)
    assert all(len(s["recall"].draws) == 1 and s["p"] == s["bp"] for s in refused) and {s["seat"] for s in refused} == {0, 1}
    assert any(w["status"] == MM.LOOKUP for w in want) and all(w["status"] in (MM.OK, MM.LOOKUP) for w in want)
    # a refused solve and a played one in the same hand; with the shared batches, every fallback a hand has been seen to reach
    both = [w for w in want if w["status"] == MM.OK and {RP.XM.SOLVE, RP.XM.SOLVED} <= {s["fallback"] for s in w["steps"]}]
    assert len(both) >= 2 and all(s["result"]["visits"].any() for w in both for s in w["steps"] if s["fallback"] == RP.XM.SOLVED)
    assert {s["fallback"] for s in kept} | {s["fallback"] for name in SC.NAMES for s in m.all_steps(name)} == {
        RP.XM.SOLVED, RP.XM.BELIEF, RP.XM.SOLVE, RP.XM.KEY}
    assert all(w["unsolved"] == sum(s["fallback"] != RP.XM.SOLVED for s in w["steps"]) for w in want if w["status"] == MM.OK)
    kw = dict(args.kwargs(), **sargs.kwargs())
    equals(pair[0].search_match(SOLVE_N, pair[1], **kw), want, SC.STEPS_CAP, "host form")
    equals(host_view(pair[0].search_match_device(SOLVE_N, pair[1], **kw), SOLVE_N), want, SC.STEPS_CAP, "device form")
    for s in pair:
        s.close()
    for t in tables:
        t.close()

"""Translation on the device: rp_nlhe_translate, host and _device forms, against the naive history walker of
tests/nlhe_translate_model.py (pinned by tests/test_nlhe_translate_model.py).  Bytes and integers only: there is no tolerance.

The hands are the records of a short blueprint-vs-fish match on a table trained three steps at batch 128 — the fish raises the
minimum, which is almost never a grid size — with the pot-12 and 3-bet hands of the contract mixed into the middle of every batch.
The encoder is the hashed one, so RP_RECALL_LOOKUP (lookup tables that do not hold an observation) cannot occur here."""
import numpy as np
import pytest
import torch

import nlhe_read_chunk as RC
import nlhe_translate_cases as TC
import nlhe_translate_model as TM
from robopoker_amd.nlhe import AIVAT_DTYPE, MAX_HOLES, RECALL_DTYPE, AivatHand, NlheSolver

pytestmark = pytest.mark.gpu

KINDS = ("snap", "harmonic", "phargmax")
FIELDS = ("recalls", "play_edges", "past", "present", "choices", "n_choices", "status")
CHUNK = 1 << 20  # the read side's launch chunk
SEED, FIRST_ID = 11, 5000


@pytest.fixture(scope="module")
def solver(gpu):
    s = NlheSolver(cap_log2=18, batch=128, seed=5, sampling="pluribus")
    for _ in range(3):
        s.step()
    yield s
    s.close()


@pytest.fixture(scope="module")
def played(solver):
    """the hands of a blueprint-vs-fish match, the model's view of them, and batches cut from them"""
    got = solver.match(257, agents=("blueprint", "fish"), seed=3, first_id=40)
    assert not got["status"].any()
    return TC.hands_of(got["hands"])


def batch(played, n):
    """n hands: the match's, the pot-12 and the 3-bet hand in the middle where there is room"""
    hands = list(played[:n])
    if n >= 3:
        hands[n // 2 - 1: n // 2 + 1] = [TC.POT12, TC.THREE_BET]
    assert len(hands) == n
    return hands


def want(hands, kind, pov=None, upto=None, first_id=FIRST_ID):
    return TC.pack(TM.recalls(hands, kind, pov, upto, SEED, first_id))


def on_host(solver, hands, kind, pov=None, upto=None, first_id=FIRST_ID):
    return solver.translate(hands, kind, pov, upto, seed=SEED, first_id=first_id)


def on_device(solver, hands, kind, pov=None, upto=None, first_id=FIRST_ID):
    dev = lambda a, dtype: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()  # noqa: E731
    out = solver.translate_device(dev(AivatHand.pack(hands).view(np.uint8).reshape(-1, AIVAT_DTYPE.itemsize), np.uint8), kind,
                                  dev(pov, np.uint8), dev(upto, np.uint8), seed=SEED, first_id=first_id)
    solver.sync()
    assert all(t.is_cuda for t in out.values())
    out = {k: v.cpu().numpy() for k, v in out.items()}
    return dict(out, recalls=out["recalls"].reshape(-1).view(RECALL_DTYPE), past=out["past"].view(np.uint64),
                present=out["present"].view(np.uint32), choices=out["choices"].view(np.uint64))


def same(got, expected, what):
    for f in FIELDS:
        assert got[f].dtype == expected[f].dtype and got[f].shape == expected[f].shape, (what, f)
        rows = [i for i in range(len(expected[f])) if got[f][i].tobytes() != expected[f][i].tobytes()]
        assert not rows, (what, f, rows[:5], got[f][rows[0]], expected[f][rows[0]])


@pytest.mark.parametrize("kind", KINDS)
def test_single_hands_through_both_forms(solver, kind):
    for name, hand in TC.SINGLES.items():
        expected = want([hand], kind)
        same(on_host(solver, [hand], kind), expected, (name, "host"))
        same(on_device(solver, [hand], kind), expected, (name, "device"))
    got = on_host(solver, [TC.POT12, TC.THREE_BET], kind)
    assert got["play_edges"][0, 4] == 12 and got["play_edges"][1, 1] in dict(snap=(15,), phargmax=(18,), harmonic=(15, 18))[kind]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", (1, 63, 64, 65, 256, 257))
def test_batches_at_wavefront_and_workgroup_edges(solver, played, kind, n):
    hands = batch(played, n)
    expected = want(hands, kind)
    assert not expected["status"].any()
    same(on_host(solver, hands, kind), expected, "host")
    if n in (1, 65, 257):
        same(on_device(solver, hands, kind), expected, "device")
    if n == 257:  # the off-tree plays are there: the three policies differ, and Snap differs from the match's own edgify history
        assert (expected["play_edges"] >= 6).sum() > 20
        assert expected["play_edges"].tobytes() != want(hands, "snap" if kind != "snap" else "phargmax")["play_edges"].tobytes()


def test_one_hand_more_than_a_launch_chunk(solver, played):
    hands = batch(played, 257)
    n, reps = CHUNK + 1, -(-(CHUNK + 1) // 257)
    packed = torch.from_numpy(AivatHand.pack(hands).view(np.uint8).reshape(257, -1)).cuda()
    tiled = packed.repeat(reps, 1)[:n].contiguous()
    expected = want(hands, "phargmax")  # no draw is read: every copy of a hand answers the same bytes
    got = solver.translate_device(tiled, "phargmax", seed=SEED, first_id=FIRST_ID)
    solver.sync()
    for f in FIELDS:
        one = torch.from_numpy(expected[f].view(np.uint8).reshape(257, -1)).cuda()
        assert torch.equal(got[f].view(torch.uint8).reshape(n, -1), one.repeat(reps, 1)[:n]), f
    # the second launch counts its hand ids on from the first.  Its one hand is the 3-bet, under an id whose harmonic draw decides
    # otherwise than the draw of the id the hand would have if the launch began at first_id again
    low = lambda hand_id: TM.uniform(SEED, hand_id, 1) < 0.4  # noqa: E731
    first_id = next(f for f in range(FIRST_ID, FIRST_ID + 64) if low(f + CHUNK) != low(f))
    tiled[n - 1] = torch.from_numpy(AivatHand.pack([TC.THREE_BET]).view(np.uint8)).cuda()
    got = solver.translate_device(tiled, "harmonic", seed=SEED, first_id=first_id)
    solver.sync()
    at = CHUNK // 257 * 257  # the last whole copy of the batch ends here, 16 hands before the cut
    last = hands[: CHUNK - at] + [TC.THREE_BET]
    assert at < CHUNK and len(last) == 17
    window = want(last, "harmonic", first_id=first_id + at)
    for f in FIELDS:
        assert got[f][at:].cpu().numpy().tobytes() == window[f].tobytes(), f
    assert window["play_edges"][16, 1] != want([TC.THREE_BET], "harmonic", first_id=first_id)["play_edges"][0, 1]


@pytest.mark.parametrize("kind", KINDS)
def test_upto_cut_at_every_play_from_both_seats(solver, kind):
    n = len(TC.MULTI_STREET.plays) + 1
    hands, upto, pov = [TC.MULTI_STREET] * n, np.arange(n, dtype=np.uint8), np.arange(n, dtype=np.uint8) % 2
    expected = want(hands, kind, pov, upto)
    assert not expected["status"].any() and expected["n_choices"][:-1].all() and expected["n_choices"][-1] == 0
    assert [int(r["n_edges"]) for r in expected["recalls"]] == sorted(int(r["n_edges"]) for r in expected["recalls"])
    same(on_host(solver, hands, kind, pov, upto), expected, "host")
    same(on_device(solver, hands, kind, pov, upto), expected, "device")
    same(on_host(solver, hands, kind, None, upto), want(hands, kind, None, upto), "pov of the hand")


def test_a_refused_hand_between_good_ones(solver, played):
    bad = TC.refusals()
    assert sorted(s for _, _, s in bad) == [TM.EDGE, TM.ILLEGAL, TM.ILLEGAL, TM.LENGTH, TM.CARDS, TM.DRAW, TM.SEAT]
    hands, pov = [], []
    for i, (hand, p, _) in enumerate(bad):
        hands += [played[2 * i], hand, played[2 * i + 1]]
        pov += [played[2 * i].seat, hand.seat if p is None else p, played[2 * i + 1].seat]
    hands.append(AivatHand(TC.HOLES, TC.DRAWS, TC.POT12.plays))
    pov.append(0)
    upto = np.array([len(h.plays) for h in hands], np.uint8)
    upto[-1] += 1  # more plays asked for than the hand has
    expected = want(hands, "phargmax", pov, upto)
    assert list(expected["status"][1::3]) == [s for _, _, s in bad] and expected["status"][-1] == TM.LENGTH
    assert not expected["status"][0:-1:3].any() and not expected["status"][2::3].any()
    for form in (on_host, on_device):
        got = form(solver, hands, "phargmax", pov, upto)
        same(got, expected, form.__name__)
        for f in FIELDS[:-1]:  # a refused hand: zero outputs
            assert not np.frombuffer(got[f][1::3].tobytes() + got[f][-1:].tobytes(), np.uint8).any(), f
    good = [h for i, h in enumerate(hands[:-1]) if i % 3 != 1]
    alone = on_host(solver, good, "snap", first_id=0)
    mixed = on_host(solver, hands, "snap", pov, upto, first_id=77)  # Snap reads no draw: the ids do not matter
    keep = [i for i in range(len(hands) - 1) if i % 3 != 1]
    for f in FIELDS:
        assert mixed[f][keep].tobytes() == alone[f].tobytes(), f


def test_a_hand_does_not_depend_on_the_batch_around_it(solver, played):
    hands = batch(played, 257)
    whole = on_host(solver, hands, "harmonic")
    same(whole, want(hands, "harmonic"), "whole")
    for at, n in ((0, 100), (100, 157), (63, 2), (256, 1)):
        part = on_device(solver, hands[at: at + n], "harmonic", first_id=FIRST_ID + at)
        for f in FIELDS:
            assert part[f].tobytes() == whole[f][at: at + n].tobytes(), (at, n, f)
    moved = on_host(solver, hands, "harmonic", first_id=FIRST_ID + 1)
    assert moved["play_edges"].tobytes() != whole["play_edges"].tobytes()


def test_match_to_translate_to_ranges_without_a_host_copy(solver):
    n, args = 48, dict(agents=("blueprint", "fish"), seed=8, first_id=900)
    dev = solver.match_device(n, **args)
    solver.sync()  # torch's stream reads the records next
    upto = dev["hands"][:, AIVAT_DTYPE.fields["n_plays"][1]] - 1  # every hand at the decision of its last play
    tr = solver.translate_device(dev["hands"], "phargmax", upto=upto)
    reach = solver.reaches_device(tr["recalls"], "opponent")
    policy = solver.policy(tr["past"], tr["present"], tr["choices"], kind="averaged")
    solver.sync()
    # the host path: the same match brought to the host, the model's recalls, the host forms of the two queries
    hands = TC.hands_of(solver.match(n, **args)["hands"])
    expected = TC.pack(TM.recalls(hands, "phargmax", upto=[len(h.plays) - 1 for h in hands]))
    assert not expected["status"].any() and expected["n_choices"].all()
    assert tr["recalls"].cpu().numpy().tobytes() == expected["recalls"].tobytes()
    raw = solver.reaches_raw(expected["recalls"], "opponent")
    assert not raw["status"].any() and raw["count"].min() > 0 and raw["reach"].shape == (n, MAX_HOLES)
    for f in ("count", "holes", "reach", "status"):
        assert reach[f].cpu().numpy().tobytes() == raw[f].tobytes(), f
    host = solver.policy(expected["past"], expected["present"], expected["choices"], kind="averaged")
    for f in ("policy", "edges", "n_actions", "found"):
        assert policy[f].cpu().numpy().tobytes() == host[f].tobytes(), f
    assert np.array_equal(host["n_actions"], expected["n_choices"]) and host["found"].any()


def test_the_table_is_untouched(solver, played):
    before = (solver.export(), solver.epoch, solver.counters())
    hands = batch(played, 65)
    for kind in KINDS:
        on_host(solver, hands, kind)
        on_device(solver, hands, kind)
    after = (solver.export(), solver.epoch, solver.counters())
    assert all(np.array_equal(x, y) for x, y in zip(before[0][:3], after[0][:3])) and before[0][3].tobytes() == after[0][3].tobytes()
    assert before[1:] == after[1:]


@pytest.mark.parametrize("kind", ("harmonic", "phargmax"))
def test_small_launch_chunks_cut_the_optional_inputs(solver, played, kind):
    """RP_NLHE_READ_CHUNK (tests/nlhe_read_chunk.py) cuts the refused-hand batch into launches of 1, 3, n - 1 and n hands: every launch
    reads pov and upto, and counts the ids of its harmonic draws, from its own hand on.  Against the model, not only against one launch"""
    bad = TC.refusals()
    hands, pov = [], []
    for i, (hand, p, _) in enumerate(bad):
        hands += [played[2 * i], hand, played[2 * i + 1]]
        pov += [1 - played[2 * i].seat, hand.seat if p is None else p, played[2 * i + 1].seat]
    hands += [TC.THREE_BET, TC.POT12]
    pov += [1, 0]
    n = len(hands)
    upto = np.array([len(h.plays) - (i % 3 == 2) for i, h in enumerate(hands)], np.uint8)  # every third hand before its last play
    upto[-1] = len(TC.POT12.plays) + 1  # more plays asked for than the hand has: refused, in a launch of its own at n - 1
    expected = want(hands, kind, pov, upto)
    assert n % 16 and list(expected["status"][1:-2:3]) == [s for _, _, s in bad] and expected["status"][-1] == TM.LENGTH
    assert expected["recalls"].tobytes() != want(hands, kind, None, upto)["recalls"].tobytes()
    assert expected["recalls"].tobytes() != want(hands, kind, pov, None)["recalls"].tobytes()
    if kind == "harmonic":  # the ids matter: counted from first_id again at the first cut of 3, some draw decides otherwise
        again = want(hands[3:], kind, pov[3:], upto[3:])
        assert again["play_edges"].tobytes() != expected["play_edges"][3:].tobytes()
    with RC.read_chunk(None):
        same(on_host(solver, hands, kind, pov, upto), expected, "one launch")
    for chunk in RC.cuts(n):
        with RC.read_chunk(chunk):
            same(on_host(solver, hands, kind, pov, upto), expected, (chunk, "host"))
            same(on_device(solver, hands, kind, pov, upto), expected, (chunk, "device"))
    with RC.read_chunk(3):  # pov and upto left out, alone and together; one hand
        same(on_host(solver, hands, kind, None, upto), want(hands, kind, None, upto), "without pov")
        same(on_device(solver, hands, kind, pov, None), want(hands, kind, pov, None), "without upto")
        same(on_device(solver, hands, kind), want(hands, kind), "without either")
    with RC.read_chunk(1):
        same(on_host(solver, hands[-2:-1], kind, pov[-2:-1], upto[-2:-1], first_id=FIRST_ID + n - 2),
             {f: expected[f][-2:-1] for f in FIELDS}, "one hand")

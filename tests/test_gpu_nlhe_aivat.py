"""AIVAT control variates from the device-resident blueprint: rp_nlhe_aivat, host and _device forms, against the naive two-game model
of tests/nlhe_aivat_model.py (pinned by tests/test_nlhe_aivat_model.py, which also asserts that the batch of tests/nlhe_aivat_cases.py
holds every case named there).  Bit patterns only: there is no tolerance.

One batch of 16 hands, a 2^10-slot table, batch = 1: valid hands of every shape the two-game replay has, with a hand the witness
refuses, one the walker refuses, a bad kind, overlapping cards and a missing street between them."""
import ctypes as C

import numpy as np
import pytest
import torch

import nlhe_aivat_cases as K
import nlhe_aivat_model as AM
import nlhe_read_chunk as RC
from robopoker_amd import _lib
from robopoker_amd.nlhe import AivatHand, NlheSolver

pytestmark = pytest.mark.gpu

FLOATS, COUNTS = ("hero", "villain", "chance", "total"), ("n_action", "n_chance")
HANDS = [h for _, h in K.CASES]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def solver(rows=None):
    """rows: load the first `rows` infosets only (room for a training step in the 1 024 slots)"""
    s = NlheSolver(cap_log2=K.CAP_LOG2, batch=1, seed=1)
    s.load(*(x[:rows] for x in K.model().table), epoch=3)
    return s


def as_map(past, present, choices, enc):
    return {(int(p), int(q), int(c)): enc[i].tobytes() for i, (p, q, c) in enumerate(zip(past, present, choices))}


def check(got, j, want, what):
    """got: the call's dict, j: the hand's place in it; want: the model's (status, hero, villain, chance, total, n_action, n_chance)"""
    assert got["status"][j] == want[0], what
    for k, f in enumerate(FLOATS):
        assert bits(got[f][j : j + 1])[0] == bits(np.float32(want[1 + k]).reshape(1))[0], (what, f, got[f][j], want[1 + k])
    assert (got["n_action"][j], got["n_chance"][j]) == want[5:], what


def test_host_form_equals_the_model(gpu):
    m, s = K.model(), solver()
    before = (s.export(), s.epoch, s.counters())
    got = s.aivat(HANDS)
    for j, name in enumerate(K.NAMES):
        check(got, j, m.want[j], name)
    # the two seats of one hand: hero <-> -villain, chance <-> -chance, total <-> -total, as bit patterns
    a, b = K.NAMES.index("streets seat 0"), K.NAMES.index("streets seat 1")
    flip = np.uint32(0x80000000)
    for x, y in (("hero", "villain"), ("villain", "hero"), ("chance", "chance"), ("total", "total")):
        assert bits(got[x])[b] == bits(got[y])[a] ^ flip and bits(got[y])[a] & ~flip, (x, y)
    # read-only
    after = (s.export(), s.epoch, s.counters())
    assert all(np.array_equal(x, y) for x, y in zip(before[0][:3], after[0][:3])) and before[0][3].tobytes() == after[0][3].tobytes()
    assert before[1:] == after[1:] == (3, (0, 0, m.table[0].size))


def test_device_form_equals_the_host_form(gpu):
    s = solver()
    host = s.aivat(HANDS)
    dev = s.aivat_device(torch.from_numpy(AivatHand.pack(HANDS).view(np.uint8).copy()).to("cuda"))
    s.sync()
    assert all(t.is_cuda for t in dev.values())
    for f in FLOATS:
        assert np.array_equal(bits(dev[f].cpu().numpy()), bits(host[f])), f
    for f in COUNTS + ("status",):
        assert np.array_equal(dev[f].cpu().numpy(), host[f]), f


def test_malformed_hands_leave_their_neighbours_alone(gpu):
    m, s = K.model(), solver()
    whole = s.aivat(HANDS)
    valid = [j for j, w in enumerate(m.want) if w[0] == AM.OK]
    assert 0 < len(valid) < len(HANDS) and any(j - 1 not in valid for j in valid[1:])
    alone = s.aivat([HANDS[j] for j in valid])
    for f in FLOATS:
        assert np.array_equal(bits(alone[f]), bits(whole[f][valid])), f
    for f in COUNTS + ("status",):
        assert np.array_equal(alone[f], whole[f][valid]), f
    refused = [j for j in range(len(HANDS)) if j not in valid]
    assert not any(whole[f][refused].view(np.uint32).any() if f in FLOATS else whole[f][refused].any() for f in FLOATS + COUNTS)


def test_a_queried_table_steps_like_one_never_queried(gpu):
    s, twin = solver(rows=32), solver(rows=32)
    s.aivat(HANDS)
    s.aivat_device(torch.from_numpy(AivatHand.pack(HANDS).view(np.uint8).copy()).to("cuda"))
    s.step()
    twin.step()
    am, bm = as_map(*s.export()), as_map(*twin.export())
    assert am.keys() == bm.keys() and len(am) > 32 and all(am[k] == bm[k] for k in am)
    assert (s.epoch, s.counters()) == (twin.epoch, twin.counters()) and s.epoch == 4


def test_arguments(gpu):
    lib = _lib.load()
    s = NlheSolver(cap_log2=K.CAP_LOG2, batch=4, seed=2)
    hd = AivatHand.pack([HANDS[K.NAMES.index("preflop fold")]])
    f = [np.zeros(1, np.float32) for _ in range(4)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for fn in (lib.rp_nlhe_aivat, lib.rp_nlhe_aivat_device):
        assert fn(s._h, 0, *[None] * 8) == _lib.RP_OK  # n = 0: no launch, whatever the pointers
        assert fn(None, 0, *[None] * 8) == _lib.RP_ERR_INVALID
    assert lib.rp_nlhe_aivat(s._h, 1, None, *map(p, f), None, None, None) == _lib.RP_ERR_INVALID
    assert lib.rp_nlhe_aivat(s._h, 1, p(hd), p(f[0]), p(f[1]), p(f[2]), None, None, None, None) == _lib.RP_ERR_INVALID
    assert b"rp_nlhe_aivat" in lib.rp_last_error()
    # n_action, n_chance and status may be NULL; an empty table has no row: nothing contributes
    assert lib.rp_nlhe_aivat(s._h, 1, p(hd), *map(p, f), None, None, None) == _lib.RP_OK
    assert not any(bits(x).any() for x in f)
    # more plays than the cap is a status, not an error; so are a seat and a board_mode that do not exist; the handle still steps
    long = AivatHand(K.HOLES, K.BOARD, [("check", 0)] * 60)
    got = s.aivat([long, AivatHand(K.HOLES, (), [("fold", 0)], seat=2), AivatHand(K.HOLES, (), [("fold", 0)], board_mode=2)])
    assert list(got["status"]) == [AM.LENGTH, AM.SEAT, AM.SEAT]
    s.step()
    assert s.epoch == 1 and s.counters()[2] > 0


def test_the_corrections_do_not_depend_on_the_launch_chunk(gpu):
    """RP_NLHE_READ_CHUNK (tests/nlhe_read_chunk.py) cuts the batch into launches of 1, 3, n - 1 and n hands: every launch reads its
    hands and writes its seven outputs from its own item on"""
    m, s = K.model(), solver()
    n = len(HANDS)
    dev_in = torch.from_numpy(AivatHand.pack(HANDS).view(np.uint8).copy()).to("cuda")
    with RC.read_chunk(None):
        want = s.aivat(HANDS)
    assert n >= 7 and len(set(want["status"])) > 3
    for chunk in RC.cuts(n):
        with RC.read_chunk(chunk):
            host, dev = s.aivat(HANDS), s.aivat_device(dev_in)
            s.sync()
        RC.same(host, want, (chunk, "host"))
        RC.same({k: v.cpu().numpy() for k, v in dev.items()}, want, (chunk, "device"))
        for j, name in enumerate(K.NAMES):  # the model itself, on every hand of every launch
            check(host, j, m.want[j], (chunk, name))
    # 15 hands and one: the one-byte arrays (n_action, n_chance, status) end off the staging arena's alignment
    with RC.read_chunk(3):
        RC.same(s.aivat(HANDS[1:]), RC.tail(want, 1), "15 hands")
    with RC.read_chunk(1):
        RC.same(s.aivat(HANDS[-1:]), RC.tail(want, n - 1), "one hand")
    # n_action, n_chance and status left out, in launches of 3
    lib, hd = _lib.load(), AivatHand.pack(HANDS)
    f = [np.zeros(n, np.float32) for _ in FLOATS]
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    with RC.read_chunk(3):
        assert lib.rp_nlhe_aivat(s._h, n, p(hd), *map(p, f), None, None, None) == _lib.RP_OK
    RC.same(f, [want[k] for k in FLOATS], "without the counts and the status")

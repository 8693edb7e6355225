"""The NLHE infoset table moved on the device (robopoker_amd/csrc/nlmc_table.hpp; rp_nlhe_capacity / _resize / _set_growth /
_export_device / _import_device): compaction against the host export, bulk insertion against the host import with data from
oracle/rp_oracle_nlmc.c, the rehash into another size under a running trainer, and growth in front of a step.

Everything compared here is compared BY KEY and BYTE FOR BYTE: a table's slot placement differs between handles (insertion order, table
size), what it holds does not.  Twin runs use seed 91 and batch 16; the CPU oracle's key counts at that seed and batch after steps
1 to 6 are 1 790, 3 631, 5 027, 8 018, 9 457, 11 621 (the most one step adds: 2 991) — the growth schedule asserted below follows
from them."""
import numpy as np
import pytest
import torch

import nlhe_policy_model as PM
import oracle_nlmc as M
from robopoker_amd import _lib
from robopoker_amd.nlhe import ENC_DTYPE, NlheSolver

pytestmark = pytest.mark.gpu
SEED, BATCH = 91, 16
ORACLE_KEYS = (1790, 3631, 5027, 8018, 9457, 11621)


def solver(cap_log2):
    return NlheSolver(cap_log2=cap_log2, batch=BATCH, seed=SEED)


def to_device(past, present, choices, enc):
    n = len(past)
    return (torch.from_numpy(np.ascontiguousarray(past, np.uint64).view(np.int64).copy()).cuda(),
            torch.from_numpy(np.ascontiguousarray(present, np.uint32).view(np.int32).copy()).cuda(),
            torch.from_numpy(np.ascontiguousarray(choices, np.uint64).view(np.int64).copy()).cuda(),
            torch.from_numpy(np.ascontiguousarray(enc, ENC_DTYPE).view(np.uint8).reshape(n, 9, 16).copy()).cuda())


def to_host(past, present, choices, enc, *_):
    return (past.cpu().numpy().view(np.uint64), present.cpu().numpy().view(np.uint32), choices.cpu().numpy().view(np.uint64),
            enc.cpu().numpy().view(ENC_DTYPE)[..., 0])


def same_map(a, b):
    return a.keys() == b.keys() and all(a[k].tobytes() == b[k].tobytes() for k in a)


def absent_keys(present_map, n=64):
    rng = np.random.default_rng(7)
    past = rng.integers(1, 1 << 62, n, dtype=np.uint64)
    present = (0x0100 | rng.integers(0, 200, n)).astype(np.uint32)
    choices = np.full(n, 6 | (5 << 5) | (4 << 10) | (2 << 15), np.uint64)
    assert all((int(p), int(b), int(c)) not in present_map for p, b, c in zip(past, present, choices))
    return past, present, choices


def answers(s, past, present, choices):
    """what the table says by key, as bytes: both stored distributions and the Encounters"""
    out = []
    for kind in ("averaged", "iterated"):
        r = s.policy(past, present, choices, kind=kind)
        out += [r[f].tobytes() for f in ("policy", "edges", "n_actions", "found")]
    enc, nact, found = s.memory(past, present, choices)
    return out + [enc.tobytes(), nact.tobytes(), found.tobytes()]


def with_absent(arrays, table_map):
    ap, ab, ac = absent_keys(table_map)
    return np.concatenate([arrays[0], ap]), np.concatenate([arrays[1], ab]), np.concatenate([arrays[2], ac])


@pytest.fixture(scope="module")
def blueprint():
    """the oracle's table after three steps, computed once and only read: (past, present, choices, enc), epoch"""
    ora = M.OracleNlhe(cap_log2=18, batch=BATCH, seed=SEED)
    for _ in range(3):
        ora.step()
    arrays = ora.export()
    assert len(arrays[0]) == ora.counters()[2] == ORACLE_KEYS[2]
    for a in arrays:
        a.setflags(write=False)
    return arrays, ora.epoch


def test_export_on_the_device_is_the_host_export(gpu):
    s = solver(14)
    assert s.export_device()[4] == 0 and s.export_device()[0].numel() == 0  # an empty table
    s.step("ordered")
    s.step("ordered")
    host = s.export()
    *dev, n = s.export_device()
    assert n == len(host[0]) == s.counters()[2] > 3000
    for h, d in zip(host, to_host(*dev)):  # the same order, keys and Encounters
        assert h.tobytes() == d.tobytes()
    for cap in (1, 100, 1025):  # a cap below n: the first cap entries and the full count
        *few, n_few = s.export_device(cap=cap)
        assert n_few == n and few[0].numel() == cap
        for h, d in zip(host, to_host(*few)):
            assert h[:cap].tobytes() == d.tobytes()


def test_import_on_the_device_with_data_from_the_oracle(gpu, blueprint):
    arrays, epoch = blueprint
    want = M.as_map(*arrays)
    s, twin = solver(14), solver(14)
    s.load_device(*to_device(*arrays), epoch)
    twin.load(*arrays, epoch=epoch)
    assert same_map(M.as_map(*s.export()), want)
    assert s.counters()[2] == s.capacity()[1] == len(want) and s.capacity()[0] == 14
    assert s.epoch == twin.epoch == epoch
    asked = with_absent(arrays, want)
    assert answers(s, *asked) == answers(twin, *asked)
    s.step("ordered")
    twin.step("ordered")
    assert s.counters() == twin.counters()
    assert same_map(M.as_map(*s.export()), M.as_map(*twin.export()))


@pytest.mark.parametrize("chunk", [None, 1000])
def test_a_key_named_again_keeps_its_last_encounters(gpu, blueprint, monkeypatch, chunk):
    # 200 keys of the batch appear a second time with other Encounters, everything in random order: the result is what the host
    # import of the same arrays leaves, whether the call is one chunk or six (RP_NLHE_IMPORT_CHUNK: items per pair of launches)
    (past, present, choices, enc), epoch = blueprint
    rng = np.random.default_rng(3)
    again = rng.choice(len(past), 200, replace=False)
    enc2 = enc[again].copy()
    enc2["regret"] += np.float32(1.5)
    enc2["weight"] *= np.float32(0.5)
    enc2["payoff"] -= np.float32(2.0)
    enc2["visits"] += 7
    order = rng.permutation(len(past) + 200)
    arrays = tuple(np.concatenate([a, b])[order] for a, b in ((past, past[again]), (present, present[again]), (choices, choices[again]), (enc, enc2)))
    s, twin = solver(14), solver(14)
    if chunk:
        monkeypatch.setenv("RP_NLHE_IMPORT_CHUNK", str(chunk))
    s.load_device(*to_device(*arrays), epoch)
    twin.load(*arrays, epoch=epoch)
    got, want = M.as_map(*s.export()), M.as_map(*twin.export())
    assert same_map(got, want)
    assert s.counters()[2] == len(got) == len(past)
    changed = sum(got[(int(past[i]), int(present[i]), int(choices[i]))].tobytes() != enc[i].tobytes() for i in again)
    assert changed > 60  # the repeat comes behind the original about every other time


@pytest.mark.parametrize("mode", ["ordered", "composed"])
def test_resize_keeps_the_blueprint_and_the_run(gpu, mode):
    s, twin = solver(14), solver(17)
    for _ in range(2):
        s.step(mode)
    before = s.export()
    table = M.as_map(*before)
    keys = len(table)
    if mode == "ordered":
        assert keys == ORACLE_KEYS[1]
    asked = with_absent(before, table)
    said, counters, epoch = answers(s, *asked), s.counters(), s.epoch

    def unchanged(cap_log2):
        assert s.capacity() == (cap_log2, keys)
        assert s.counters() == counters and s.epoch == epoch
        assert same_map(M.as_map(*s.export()), table)
        assert answers(s, *asked) == said

    s.resize(17)
    unchanged(17)
    s.resize(17)  # the same size: nothing to do
    unchanged(17)
    s.resize(13)  # back down: 2 * keys <= 8 192
    unchanged(13)
    with pytest.raises(_lib.RpError) as e:
        s.resize(12)
    assert e.value.code == 5
    unchanged(13)
    s.resize(17)
    for _ in range(2):
        s.step(mode)
    for _ in range(4):
        twin.step(mode)
    assert s.counters() == twin.counters() and s.epoch == twin.epoch == 4
    assert same_map(M.as_map(*s.export()), M.as_map(*twin.export()))


def _homed_at_the_end(arrays, cap_log2, last):
    """the indices of the keys whose probe starts in the last `last` slots of a table of 2^cap_log2"""
    mask = (1 << cap_log2) - 1
    return [i for i, (p, b, c) in enumerate(zip(*arrays[:3])) if PM.key_hash(p, c, b) & mask > mask - last]


def _holds(s, arrays):
    enc, nact, found = s.memory(*arrays[:3])
    live = np.arange(9)[None, :] < nact[:, None]
    want = np.array(arrays[3], dtype=ENC_DTYPE)  # Source::memory answers zero in the slots behind the infoset's actions
    want[~live] = np.zeros((), ENC_DTYPE)
    return bool(found.all()) and enc.tobytes() == want.tobytes()


def test_long_probe_chains_and_the_wrap_at_the_tables_end(gpu, blueprint):
    arrays, epoch = blueprint
    # 250 keys in 256 slots: chains through most of the table and round its end, in the insertion
    first = tuple(a[:250] for a in arrays)
    s = solver(8)
    s.load_device(*to_device(*first), epoch)
    assert s.capacity() == (8, 250) and _holds(s, first)
    s.resize(9)
    assert s.capacity() == (9, 250) and _holds(s, first)
    with pytest.raises(_lib.RpError) as e:  # 2 * 250 > 256: refused before anything is allocated
        s.resize(8)
    assert e.value.code == 5 and s.capacity() == (9, 250) and _holds(s, first)
    # 120 keys, 100 of them homed in the last 16 slots of a 256-slot table and more than 16 in the last 16 of a 512-slot one: the
    # insertion, the rehash up and the rehash back down each carry a chain round the end of their table
    end8, end9 = _homed_at_the_end(arrays, 8, 16), _homed_at_the_end(arrays, 9, 16)
    pick = [i for i in end9 if i in set(end8)][:40]
    pick += [i for i in end8 if i not in set(pick)][: 100 - len(pick)]
    assert len(pick) == 100 and len([i for i in pick if i in set(end9)]) > 16
    pick += [i for i in range(len(arrays[0])) if i not in set(pick)][:20]
    crowd = tuple(a[pick] for a in arrays)
    t = solver(8)
    t.load_device(*to_device(*crowd), epoch)
    assert t.capacity() == (8, 120) and _holds(t, crowd)
    t.resize(9)
    assert t.capacity() == (9, 120) and _holds(t, crowd)
    t.resize(8)
    assert t.capacity() == (8, 120) and _holds(t, crowd)
    assert same_map(M.as_map(*t.export()), M.as_map(*crowd))
    # 300 distinct keys do not fit 256 slots: an error code from a bounded probe loop, and the handle goes on answering
    full = solver(8)
    with pytest.raises(_lib.RpError) as e:
        full.load_device(*to_device(*(a[:300] for a in arrays)), epoch)
    assert e.value.code == 5 and full.epoch == 0
    assert full.capacity() == (8, 256)


def test_growth_in_front_of_a_step(gpu):
    s, twin, fixed, trained = solver(12), solver(18), solver(12), solver(12)
    s.set_growth(16, headroom=4096)
    sizes = []
    for _ in range(6):
        s.step("ordered")
        twin.step("ordered")
        sizes.append(s.capacity()[0])
    # 2 * (keys + 4 096) > slots with the oracle's counts: 2^13 before step 1, 2^14 before step 2, 2^15 before step 4
    assert sizes == [13, 14, 14, 15, 15, 15]
    assert s.capacity() == (15, twin.counters()[2]) and twin.counters()[2] == ORACLE_KEYS[5]
    assert s.counters() == twin.counters() and s.epoch == twin.epoch == 6
    want = M.as_map(*twin.export())
    assert same_map(M.as_map(*s.export()), want)
    # growth is off unless asked for: 2^12 slots are full in the third step, as ever
    fixed.step("ordered")
    fixed.step("ordered")
    with pytest.raises(_lib.RpError) as e:
        fixed.step("ordered")
    assert e.value.code == 5 and "32" in str(e.value)
    # the trainer loop grows like the single steps
    trained.set_growth(16, headroom=4096)
    trained.train("ordered", max_steps=6)
    assert trained.capacity() == s.capacity() and trained.counters() == s.counters()
    assert same_map(M.as_map(*trained.export()), want)
    for bad in (11, 31):
        with pytest.raises(_lib.RpError) as e:
            fixed.set_growth(bad)
        assert e.value.code == _lib.RP_ERR_INVALID


def test_growth_on_import(gpu, blueprint):
    arrays, epoch = blueprint
    s = solver(10)
    s.set_growth(16)
    s.load_device(*to_device(*arrays), epoch)
    assert s.capacity() == (14, ORACLE_KEYS[2]) and s.epoch == epoch
    assert same_map(M.as_map(*s.export()), M.as_map(*arrays))

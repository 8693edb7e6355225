"""Policy and Encounter queries BY NlheInfo KEY against the device-resident blueprint table (rp_nlhe_policy / rp_nlhe_memory and
their _device forms), and the same distributions of a row-addressed table (rp_profile_policy).

Every comparison is on bit patterns against tests/nlhe_policy_model.py, which tests/test_nlhe_policy_model.py pins to the CPU
oracle: there is no tolerance.  What the queries must get right: the probe chain (keys off their home slot, chains that wrap past
the last slot, a completely full table, absent keys that differ from a present one in a single field), the defaults of an absent
infoset, zeros beyond the infoset's actions whatever the row holds there, the float order, and that nothing is written."""
import ctypes as C

import numpy as np
import pytest
import torch

import nlhe_policy_model as PM
from robopoker_amd import _lib
from robopoker_amd.mccfr import default_hyper
from robopoker_amd.nlhe import A, ENC_DTYPE, NlheSolver
from robopoker_amd.sparse import SparseProfile

pytestmark = pytest.mark.gpu

KINDS = ("iterated", "averaged", "sampling")
CAP_LOG2 = 8  # 256 slots: the smallest table rp_nlhe_create allows
SLOTS = 1 << CAP_LOG2
CRAFT_SEED = 3  # with this seed keys sit off their home slot AND a probe chain wraps past slot 255 (asserted below)
REGRETS = np.array([-4e6, -1.0, 0.0, 1e-30, 3.5, 1e30], np.float32)
WEIGHTS = np.array([0.0, 1e-39, 1.0, 1e12], np.float32)  # 1e-39 is subnormal: below RP_EPSILON


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def hyper_kw(hp):
    return dict(temperature=hp.temperature, smoothing=hp.smoothing, curiosity=hp.curiosity)


def random_keys(rng, n):
    """n distinct NlheInfo keys: past below 2^63, present below 2^16, choices = 1..9 edge codes in 2..15"""
    past = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    present = rng.integers(0, 1 << 16, n, dtype=np.uint32)
    choices = np.zeros(n, np.uint64)
    for i in range(n):
        for a in range(int(rng.integers(1, A + 1))):
            choices[i] |= np.uint64(int(rng.integers(2, 16)) << (5 * a))
    assert len({(int(p), int(q), int(c)) for p, q, c in zip(past, present, choices)}) == n
    return past, present, choices


def random_rows(rng, choices):
    """Encounters from the corner values; the slots beyond each infoset's actions hold garbage (7.0 / 7)"""
    n = choices.size
    enc = np.zeros((n, A), dtype=ENC_DTYPE)
    enc["regret"] = rng.choice(REGRETS, (n, A))
    enc["weight"] = rng.choice(WEIGHTS, (n, A))
    enc["payoff"] = rng.standard_normal((n, A)).astype(np.float32) * 100
    enc["visits"] = rng.integers(0, 1 << 32, (n, A), dtype=np.uint32)
    enc["regret"][0] = rng.choice(REGRETS[:2], A)  # every regret negative: the iterated distribution is uniform
    dead = np.arange(A)[None, :] >= PM.nch_rows(choices)[:, None]
    for f in ("weight", "regret", "payoff", "visits"):
        enc[f][dead] = 7
    return enc


def placement(past, present, choices):
    """slot of every key after rp_nlhe_import into an empty table (insertion in order, linear probing), from the model's hash"""
    taken, slot, home = set(), [], []
    for p, q, c in zip(past, present, choices):
        h = PM.key_hash(p, c, q) & (SLOTS - 1)
        s = h
        while s in taken:
            s = (s + 1) & (SLOTS - 1)
        taken.add(s)
        slot.append(s)
        home.append(h)
    return np.array(slot), np.array(home)


def absent_keys(past, present, choices, n):
    """n keys that are NOT in the table and each differ from a loaded key in one field only: half another present, half another past"""
    half = n // 2
    a = (past[:half], present[:half] ^ np.uint32(1 << 16), choices[:half])
    b = (past[half:n] ^ np.uint64(1 << 63), present[half:n], choices[half:n])
    return tuple(np.concatenate([x, y]) for x, y in zip(a, b))


def expected(keys, enc_of_key, found, hp):
    """model answers for the (unique) keys: dict kind -> policy, plus memory, edges, n_actions"""
    kw = hyper_kw(hp)
    out = {k: PM.policy_rows(k, keys[2], enc_of_key, found, **kw) for k in KINDS}
    out["memory"] = PM.memory_rows(keys[2], enc_of_key, found)
    out["edges"] = PM.edges_rows(keys[2])
    out["n_actions"] = PM.nch_rows(keys[2])
    out["found"] = np.asarray(found, bool)
    return out


def check_policy(got, want, pick, kind, what=""):
    assert np.array_equal(bits(got["policy"]), bits(want[kind][pick])), (what, kind)
    assert np.array_equal(got["edges"], want["edges"][pick]), (what, kind)
    assert np.array_equal(got["n_actions"], want["n_actions"][pick]), (what, kind)
    assert np.array_equal(got["found"], want["found"][pick]), (what, kind)


def check_memory(got, want, pick, what=""):
    enc, nact, found = got
    assert enc.tobytes() == np.ascontiguousarray(want["memory"][pick]).tobytes(), what
    assert np.array_equal(nact, want["n_actions"][pick]) and np.array_equal(found, want["found"][pick]), what


class Crafted:
    """a 256-slot table with `n_keys` crafted infosets, a query list (every key, `n_absent` absent keys, duplicates; shuffled) and the
    model's answers — built once per module"""

    def __init__(self, n_keys, n_absent, n_queries, seed):
        rng = np.random.default_rng(seed)
        self.hp = default_hyper()
        self.keys = random_keys(rng, n_keys)
        self.enc = random_rows(rng, self.keys[2])
        self.slot, self.home = placement(*self.keys)
        absent = absent_keys(*self.keys, n_absent)
        pool = tuple(np.concatenate([k, a]) for k, a in zip(self.keys, absent))
        found = np.arange(n_keys + n_absent) < n_keys
        enc_pool = np.concatenate([self.enc, np.zeros((n_absent, A), dtype=ENC_DTYPE)])
        self.want = expected(pool, enc_pool, found, self.hp)
        self.pick = np.concatenate([np.arange(n_keys + n_absent), rng.integers(0, n_keys + n_absent, n_queries - n_keys - n_absent)])
        rng.shuffle(self.pick)
        self.q = tuple(k[self.pick] for k in pool)

    def solver(self):
        s = NlheSolver(cap_log2=CAP_LOG2, batch=1, seed=1, hyper=self.hp)
        s.load(*self.keys, self.enc, epoch=3)
        return s


@pytest.fixture(scope="module")
def crafted():
    return Crafted(200, 100, 1000, CRAFT_SEED)


@pytest.fixture(scope="module")
def full():
    return Crafted(SLOTS, 50, SLOTS + 50, CRAFT_SEED + 1)


def test_crafted_table_probe_chains_and_wrap_around(gpu, crafted):
    c = crafted
    assert (c.slot != c.home).any(), "no key sits off its home slot: pick another CRAFT_SEED"
    assert (c.slot < c.home).any(), "no probe chain wraps past the last slot: pick another CRAFT_SEED"
    assert np.allclose(c.want["iterated"][0][: c.want["n_actions"][0]], 1.0 / c.want["n_actions"][0])  # the all-negative row
    s = c.solver()
    for n in (1, 63, 65, 257, 1000):
        q = tuple(k[:n] for k in c.q)
        for kind in KINDS:
            check_policy(s.policy(*q, kind=kind), c.want, c.pick[:n], kind, n)
        check_memory(s.memory(*q), c.want, c.pick[:n], n)
    assert s.counters()[2] == 200 and s.epoch == 3


def test_one_lane_per_query_kernel_gives_the_same_answers(gpu, crafted, monkeypatch):
    # the kernel shape the shipped one is measured against (RP_NLHE_QUERY_SHAPE=lane, read at every call)
    monkeypatch.setenv("RP_NLHE_QUERY_SHAPE", "lane")
    c = crafted
    s = c.solver()
    for n in (1, 257, 1000):
        for kind in KINDS:
            check_policy(s.policy(*(k[:n] for k in c.q), kind=kind), c.want, c.pick[:n], kind, n)


def test_full_table(gpu, full):
    # every slot is taken: a probe for an absent key walks the whole table and must stop after 256 probes
    c = full
    s = c.solver()
    assert s.counters()[2] == SLOTS
    assert c.want["found"][c.pick].sum() == SLOTS and (~c.want["found"][c.pick]).sum() == 50
    for kind in KINDS:
        check_policy(s.policy(*c.q, kind=kind), c.want, c.pick, kind)
    check_memory(s.memory(*c.q), c.want, c.pick)


@pytest.fixture(scope="module")
def trained(gpu):
    s = NlheSolver(cap_log2=18, batch=128, seed=5, sampling="pluribus")
    for _ in range(3):
        s.step()
    return s


def test_trained_table(trained):
    s = trained
    before = (s.counters()[2], s.epoch)
    past, present, choices, enc = s.export()
    assert past.size > 1000
    want = expected((past, present, choices), enc, np.ones(past.size, bool), s.hp)
    everything = np.arange(past.size)
    for kind in KINDS:
        check_policy(s.policy(past, present, choices, kind=kind), want, everything, kind)
    check_memory(s.memory(past, present, choices), want, everything)
    # read-only: the key count, the epoch and the whole table are what they were
    assert (s.counters()[2], s.epoch) == before
    again = s.export()
    assert all(np.array_equal(x, y) for x, y in zip(again[:3], (past, present, choices))) and again[3].tobytes() == enc.tobytes()
    # the traversal's own policy_vector: each Decisions row of the current epoch carries the iterated distribution of its infoset
    b = s.batch()
    assert b["n"] == b["past"].size > 100
    got = s.policy(b["past"], b["present"], b["choices"], kind="iterated")
    assert got["found"].all() and np.array_equal(got["n_actions"], b["n_actions"])
    assert np.array_equal(bits(got["policy"]), bits(b["policy"]))


def dev_keys(q):
    return (torch.from_numpy(q[0].view(np.int64)).to("cuda"), torch.from_numpy(q[1].view(np.int32)).to("cuda"),
            torch.from_numpy(q[2].view(np.int64)).to("cuda"))


def test_device_pointer_forms(gpu, crafted, trained):
    c = crafted
    s = c.solver()
    dq = dev_keys(c.q)
    for kind in KINDS:
        got = s.policy(*dq, kind=kind)
        s.sync()
        assert all(t.is_cuda for t in got.values())
        check_policy({k: t.cpu().numpy() for k, t in got.items()}, c.want, c.pick, kind)
    enc, nact, found = s.memory(*dq)
    s.sync()
    check_memory((enc.cpu().numpy().view(ENC_DTYPE)[..., 0], nact.cpu().numpy(), found.cpu().numpy()), c.want, c.pick)
    # ordered on the solver's stream: a query queued behind a step sees the table after the step
    t = trained
    past, present, choices, _ = t.export()
    dk = dev_keys((past, present, choices))
    old = t.policy(past, present, choices, kind="averaged")["policy"]
    t.step()
    got = t.policy(*dk, kind="averaged")["policy"]
    t.sync()
    new = t.policy(past, present, choices, kind="averaged")["policy"]
    assert np.array_equal(bits(got.cpu().numpy()), bits(new)) and not np.array_equal(bits(new), bits(old))


@pytest.mark.parametrize("width", [9, 16])
def test_row_addressed_profile_policy(gpu, width):
    rng = np.random.default_rng(width)
    hp = default_hyper()
    hp.temperature, hp.smoothing, hp.curiosity = 0.7, 1.5, 0.1
    n_rows = 300
    prof = SparseProfile(n_rows, width, hyper=hp)
    enc = np.zeros((n_rows, width), dtype=ENC_DTYPE)
    enc["regret"] = rng.choice(REGRETS, (n_rows, width))
    enc["weight"] = rng.choice(WEIGHTS, (n_rows, width))
    enc["regret"][0] = -1.0
    prof.set_rows(np.arange(n_rows), enc)
    for n in (1, 257):
        rows = rng.integers(0, n_rows, n).astype(np.uint32)
        rows[0] = 0
        nact = rng.integers(0, width + 1, n).astype(np.uint8)
        nact[0] = width
        for kind in KINDS:
            got = prof.policy(rows, nact, kind)
            prof.sync()
            want = PM.distribution_rows(kind, enc["regret" if kind == "iterated" else "weight"][rows], nact, **hyper_kw(hp))
            assert got.shape == (n, width) and np.array_equal(bits(got.cpu().numpy()), bits(want)), (n, kind)


def test_errors_leave_the_handle_usable(gpu):
    lib = _lib.load()
    s = NlheSolver(cap_log2=12, batch=4, seed=2)
    k = (np.zeros(3, np.uint64), np.zeros(3, np.uint32), np.full(3, 2 | (4 << 5), np.uint64))
    pol = np.zeros((3, A), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.rp_nlhe_policy(s._h, 7, 3, p(k[0]), p(k[1]), p(k[2]), p(pol), None, None, None) == _lib.RP_ERR_INVALID
    assert b"kind" in lib.rp_last_error()
    assert lib.rp_nlhe_policy(s._h, 1, 3, None, None, None, p(pol), None, None, None) == _lib.RP_ERR_INVALID
    assert lib.rp_nlhe_policy(s._h, 1, 3, p(k[0]), p(k[1]), p(k[2]), None, None, None, None) == _lib.RP_ERR_INVALID
    assert lib.rp_nlhe_memory(s._h, 3, None, None, None, None, None, None) == _lib.RP_ERR_INVALID
    assert lib.rp_nlhe_policy_device(s._h, 7, 3, None, None, None, None, None, None, None) == _lib.RP_ERR_INVALID
    assert lib.rp_nlhe_policy(None, 1, 0, None, None, None, None, None, None, None) == _lib.RP_ERR_INVALID
    for fn in (lib.rp_nlhe_policy, lib.rp_nlhe_policy_device):
        assert fn(s._h, 1, 0, None, None, None, None, None, None, None) == _lib.RP_OK
    for fn in (lib.rp_nlhe_memory, lib.rp_nlhe_memory_device):
        assert fn(s._h, 0, None, None, None, None, None, None) == _lib.RP_OK
    assert lib.rp_profile_policy(None, 1, 0, None, None, None) == _lib.RP_ERR_INVALID
    # an absent key on an empty table answers with the defaults, and the handle still steps
    got = s.policy(*k, kind="iterated")
    assert not got["found"].any() and np.array_equal(bits(got["policy"][0, :2]), bits(np.float32([100.0, 50.0]) / np.float32(150.0)))
    s.step()
    assert s.epoch == 1 and s.counters()[2] > 0

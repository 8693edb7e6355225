"""The abstraction atlas (robopoker_amd/csrc/atlas.hip, atlas.hpp) bit for bit against tests/atlas_model.py, on the smallest tables
at which each piece can go wrong:
  (a) the preflop, 169 rows, K = 169, identity buckets: every population 1, 11 descents in obs;
  (b) flop pockets [0, 8), 6 212 rows, hashed into K = 7 and into K = 256 with every odd bucket empty (the EMPTY paths): row order and
      obs order disagree; the sort in its one-to-few-tiles regime;
  (c) turn pockets [0, 8), 65 952 rows, K = 200: several tiles, more than one workgroup per pass;
  (d) the whole flop list, 1 286 792 rows, K = 256: the sort's scanned-offsets regime; population, position and members only, against
      np.lexsort (under RP_EMUL=1 a 40-pocket prefix: the host execution model is too slow for the full list).
future / tri are synthetic (random counts with all-zero centroids and one centroid whose densities tie; distances in multiples of 1/8
so that ties decide the top k both ways).  The chain is river prefix -> (c) -> (b) -> (a).  Also runs under RP_EMUL=1 RP_EMUL_GUARD=1."""
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import atlas_model as AM  # noqa: E402
import oracle_deuce as od  # noqa: E402

F = np.float32
U64 = (1 << 64) - 1


def hashed(obs, mod):
    return ((obs.astype(np.uint64) * np.uint64(2654435761)) >> np.uint64(20)) % np.uint64(mod)


def synthetic_future(K, bins, seed):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 40, (K, bins)).astype(np.uint32) * (rng.random((K, bins)) < 0.5)
    f[1 % K] = 0  # centroids without a transition row (4 % K is a populated bucket in every case)
    f[4 % K] = 0
    f[K - 1] = 0
    f[2 % K] = 0
    f[2 % K, ::3] = 5  # every density of this centroid ties: the stable order over the bin decides the fold
    return f.astype(np.uint32), f.sum(axis=1).astype(np.uint64)


def synthetic_tri(K, seed):
    return (np.random.default_rng(seed).integers(0, 9, K * (K - 1) // 2) / 8.0).astype(F)


class Case:
    def __init__(self, name, street, obs, labels, K, below=None, row_equity=None, seed=0):
        from robopoker_amd.atlas import Atlas
        self.name, self.street, self.obs, self.labels, self.K = name, street, obs, labels.astype(np.uint8), K
        self.future = self.weight = self.tri = None
        if street < 3:
            self.future, self.weight = synthetic_future(K, below.K, seed)
            self.tri = synthetic_tri(K, seed + 1)
        self.model = AM.Atlas(street, obs, self.labels, K, self.future, self.weight, self.tri, row_equity, below.model if below else None)
        self.dev = Atlas(street, torch.from_numpy(obs).to("cuda"), torch.from_numpy(self.labels).to("cuda"), K, self.future, self.weight, self.tri,
                         None if row_equity is None else torch.from_numpy(row_equity).to("cuda"), below.dev if below else None)


@pytest.fixture(scope="module")
def cases(gpu):
    pocket = next(p for p in range(1326) if od.isomorphisms("rive", p, p + 1, count_only=True))
    rive = od.isomorphisms("rive", pocket, pocket + 1)[:5000]  # a prefix of a street's list is a valid table
    eq = np.random.default_rng(5).random(rive.size).astype(F)
    r = Case("river", 3, rive, hashed(rive, 101), 101, row_equity=eq)
    turn = od.isomorphisms("turn", 0, 8)
    c = Case("c", 2, turn, hashed(turn, 200), 200, r, seed=10)
    flop = od.isomorphisms("flop", 0, 8)
    b7 = Case("b7", 1, flop, hashed(flop, 7), 7, c, seed=20)
    b256 = Case("b256", 1, flop, hashed(flop, 128) * np.uint64(2), 256, c, seed=30)
    pref = od.isomorphisms("pref")
    a = Case("a", 0, pref, np.arange(169), 169, b256, seed=40)
    assert (turn.size, flop.size, pref.size) == (65_952, 6_212, 169)
    assert int((np.diff(flop) < 0).sum()) == 533 and int((np.diff(pref) < 0).sum()) == 11  # table order is not the BIGINT order
    assert (b256.model.population == 0).sum() >= 128 and (a.model.population == 1).all()
    out = {x.name: x for x in (r, c, b7, b256, a)}
    yield out
    for x in out.values():
        x.dev.close()


NAMES = ("a", "b7", "b256", "c", "river")


def same_bytes(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(np.frombuffer(got.tobytes(), np.uint8) != np.frombuffer(want.tobytes(), np.uint8))[:4] // max(got.dtype.itemsize, 1)
        raise AssertionError(f"first differences at elements {bad.tolist()}: got {got.reshape(-1)[bad]}, want {want.reshape(-1)[bad]}")


def relabel(rng, obs: int) -> int:
    """the same observation under a random suit permutation"""
    perm = rng.sample(range(4), 4)
    po, pu = AM.decode(obs)
    move = lambda h: sum(1 << ((c // 4) * 4 + perm[c % 4]) for c in range(52) if h >> c & 1)  # noqa: E731
    return od.obs_i64(move(po), move(pu))


def some_obs(case, rng, n):
    """table rows under random suit labellings, and absent ones: nothing, another street's, one with a repeated card"""
    rows = [rng.randrange(case.obs.size) for _ in range(n)]
    obs = [relabel(rng, int(case.obs[i])) for i in rows]
    absent = [0, -5, int(case.obs[0]) >> 8 if case.street else (int(case.obs[0]) << 8 | 9), (int(case.obs[0]) & ~0xFF) | (int(case.obs[0]) >> 8 & 0xFF)]
    if case.street:  # pocket 1325 (the two highest cards) is outside pockets [0, 8)
        absent.append(int(od.isomorphisms(case.street, 1325, 1326)[0]))
    return np.array(obs + absent, np.int64)


@pytest.mark.parametrize("name", NAMES)
def test_derived_tables(cases, name):
    c = cases[name]
    t, m = c.dev.tables(), c.model
    for f in ("population", "offset", "position", "members"):
        same_bytes(t[f], getattr(m, f))
    same_bytes(t["equity"], m.equity)
    assert int(t["population"].sum()) == c.obs.size
    td = c.dev.tables_device()
    for f in t:
        same_bytes(td[f].cpu().numpy().view(t[f].dtype), t[f])


def test_whole_flop_list_scanned_offsets(gpu):
    from robopoker_amd import deuce
    from robopoker_amd.atlas import Atlas
    big = os.environ.get("RP_EMUL") != "1"
    obs_d = deuce.isomorphisms("flop") if big else deuce.isomorphisms("flop", 0, 40)
    obs = obs_d.cpu().numpy()
    assert obs.size == 1_286_792 or not big
    labels = hashed(obs, 256).astype(np.uint8)
    # a flop atlas needs a `next` of street 2 with K = bins, and that one a river: 64-row prefixes under zero futures
    turn_obs = od.isomorphisms("turn", 0, 8)[:64].copy()
    pocket = next(p for p in range(1326) if od.isomorphisms("rive", p, p + 1, count_only=True))
    r = Atlas("rive", torch.from_numpy(od.isomorphisms("rive", pocket, pocket + 1)[:64].copy()).to("cuda"), torch.zeros(64, dtype=torch.uint8, device="cuda"), 3)
    t = Atlas("turn", torch.from_numpy(turn_obs).to("cuda"), torch.zeros(64, dtype=torch.uint8, device="cuda"), 2, np.zeros((2, 3), np.uint32),
              np.zeros(2, np.uint64), below=r)
    a = Atlas("flop", obs_d, torch.from_numpy(labels).to("cuda"), 256, np.zeros((256, 2), np.uint32), np.zeros(256, np.uint64), below=t)
    got = a.tables()
    order = np.lexsort((obs, labels)).astype(np.uint32)  # by abs, then obs
    population = np.bincount(labels, minlength=256).astype(np.uint32)
    offset = np.concatenate([[0], np.cumsum(population)]).astype(np.uint32)
    position = np.zeros(obs.size, np.uint32)
    position[order] = np.arange(obs.size, dtype=np.uint32) - offset[labels[order]]
    same_bytes(got["members"], order)
    same_bytes(got["population"], population)
    same_bytes(got["offset"], offset)
    same_bytes(got["position"], position)
    for x in (a, t, r):
        x.close()


@pytest.mark.parametrize("name", NAMES)
def test_describe(cases, name):
    c, rng = cases[name], random.Random(1)
    obs = some_obs(c, rng, 200)
    got, want = c.dev.describe(obs), c.model.describe(obs)
    same_bytes(got[0], want[0].view(got[0].dtype))
    same_bytes(got[1], want[1])
    assert (got[1][:200] == AM.OK).all() and (got[1][200:] == AM.MISS).all()
    if c.street == 3:
        return
    wrt = np.array([rng.randrange(c.K) for _ in obs], np.uint8)
    wrt[:40] = c.model.describe(obs[:40])[0]["abs"] & 0xFF  # the observation's own bucket: SAME
    if c.K < 256:
        wrt[50] = c.K  # out of range
    got, want = c.dev.describe(obs, wrt), c.model.describe(obs, wrt)
    same_bytes(got[0], want[0].view(got[0].dtype))
    same_bytes(got[1], want[1])
    assert (got[1][:40] == AM.SAME).all()


@pytest.mark.parametrize("name", NAMES)
def test_pick(cases, name):
    c, rng = cases[name], random.Random(2)
    ks = list(range(c.K)) * 3 + ([c.K] if c.K < 256 else [])
    draws = [0] * c.K + [U64] * c.K + [rng.getrandbits(64) for _ in range(len(ks) - 2 * c.K)]
    got, want = c.dev.pick(ks, np.array(draws, np.uint64)), c.model.pick(ks, draws)
    same_bytes(got[0], want[0].view(got[0].dtype))
    same_bytes(got[1], want[1])
    pop = c.model.population
    assert (got[0]["position"][:c.K] == 0).all() and (got[0]["position"][c.K:2 * c.K] == np.maximum(pop, 1) - 1).all()
    assert ((got[1][:c.K] == AM.EMPTY) == (pop == 0)).all()


@pytest.mark.parametrize("name", ("a", "b7", "b256", "c"))
@pytest.mark.parametrize("farthest", (False, True))
def test_neighbors(cases, name, farthest):
    c, rng = cases[name], random.Random(3)
    wrt = np.array(list(range(0, c.K, max(1, c.K // 24))) + ([c.K] if c.K < 256 else []), np.uint8)
    for k in (1, 6, min(c.K - 1, 16)):
        got, want = c.dev.neighbors(wrt, k, farthest), c.model.neighbors(wrt, k, farthest)
        same_bytes(got[0], want[0].view(got[0].dtype))
        same_bytes(got[1], want[1])
        draws = np.array([[rng.choice((0, U64, rng.getrandbits(64))) for _ in range(k)] for _ in wrt], np.uint64)
        got, want = c.dev.neighbors(wrt, k, farthest, draws), c.model.neighbors(wrt, k, farthest, draws.tolist())
        same_bytes(got[0], want[0].view(got[0].dtype))
        same_bytes(got[1], want[1])
    d = got[0]["distance"][0]
    assert (np.diff(d) <= 0).all() if farthest else (np.diff(d) >= 0).all()
    assert len(set(d.tolist())) < len(d)  # the quantised metric ties inside the top 16: the index decided


@pytest.mark.parametrize("name", ("a", "b7", "b256", "c"))
def test_distance(cases, name):
    c, rng = cases[name], random.Random(4)
    a = np.array([rng.randrange(c.K) for _ in range(300)], np.uint8)
    b = np.array([rng.randrange(c.K) for _ in range(300)], np.uint8)
    b[:20] = a[:20]
    if c.K < 256:
        a[25], b[26] = c.K, 255
    same_bytes(c.dev.distance(a, b), c.model.distance(a, b))


@pytest.mark.parametrize("name", NAMES)
def test_members_windows(cases, name):
    c = cases[name]
    pop = c.model.population
    ks, starts = [], []
    for k in list(range(min(c.K, 24))) + ([c.K] if c.K < 256 else []):
        p = int(pop[k]) if k < c.K else 0
        for s in (0, max(p - 3, 0), p, p + 5):  # inside, straddling the bucket's end, at it, past it
            ks.append(k)
            starts.append(s)
    for count in (1, 6, 16):
        got, want = c.dev.members(ks, starts, count), c.model.window(ks, starts, count)
        same_bytes(got[0], want[0])
        same_bytes(got[1], want[1])


@pytest.mark.parametrize("name", NAMES)
def test_obs_equity(cases, name):
    c, rng = cases[name], random.Random(6)
    obs = some_obs(c, rng, 300)
    if c.street < 3:  # a member of a bucket whose centroid has no transition row
        obs = np.append(obs, c.obs[c.model.bucket[4 % c.K][0]])
    got, want = c.dev.obs_equity(obs), c.model.obs_equity(obs)
    same_bytes(got[0], want[0])
    same_bytes(got[1], want[1])
    assert c.street == 3 or (got[1][-1] == AM.EMPTY and got[0][-1] == 0)


@pytest.mark.parametrize("name", ("a", "b7", "b256", "c"))
def test_histograms(cases, name):
    c, rng = cases[name], random.Random(7)
    ks = np.array(list(range(c.K)) + ([c.K] if c.K < 256 else []), np.uint8)
    got, want = c.dev.histograms("abs", ks), c.model.histograms(AM.HIST_ABS, ks)
    same_bytes(got[0], want[0])
    same_bytes(got[1], want[1])
    assert got[1][1 % c.K] == AM.EMPTY and not got[0][1 % c.K].any()
    obs = some_obs(c, rng, 150)
    got, want = c.dev.histograms("obs", obs), c.model.histograms(AM.HIST_OBS, obs)
    same_bytes(got[0], want[0])
    same_bytes(got[1], want[1])


@pytest.mark.parametrize("name", ("b256", "c"))
def test_device_forms_and_split_batches(cases, name):
    c, rng = cases[name], random.Random(8)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")  # noqa: E731
    host = lambda t: t.cpu().numpy()  # noqa: E731
    obs = some_obs(c, rng, 97)
    wrt = np.array([rng.randrange(c.K) for _ in obs], np.uint8)
    ks = np.array([rng.randrange(c.K) for _ in range(101)], np.uint8)
    draw = np.array([rng.getrandbits(64) for _ in ks], np.uint64)
    draws = np.array([[rng.getrandbits(64) for _ in range(6)] for _ in ks], np.uint64)
    starts = np.array([rng.randrange(40) for _ in ks], np.uint32)
    half = 50
    pairs = [
        (c.dev.describe(obs, wrt), c.dev.describe_device(dev(obs), dev(wrt)), lambda s: c.dev.describe(obs[s], wrt[s])),
        (c.dev.obs_equity(obs), c.dev.obs_equity_device(dev(obs)), lambda s: c.dev.obs_equity(obs[s])),
        (c.dev.pick(ks, draw), c.dev.pick_device(dev(ks), dev(draw.view(np.int64))), lambda s: c.dev.pick(ks[s], draw[s])),
        (c.dev.neighbors(ks, 6, True, draws), c.dev.neighbors_device(dev(ks), 6, True, dev(draws.view(np.int64))),
         lambda s: c.dev.neighbors(ks[s], 6, True, draws[s])),
        (c.dev.histograms("obs", obs), c.dev.histograms_device("obs", dev(obs)), lambda s: c.dev.histograms("obs", obs[s])),
        (c.dev.histograms("abs", ks), c.dev.histograms_device("abs", dev(ks)), lambda s: c.dev.histograms("abs", ks[s])),
        (c.dev.members(ks, starts, 5), c.dev.members_device(dev(ks), dev(starts.view(np.int32)), 5), lambda s: c.dev.members(ks[s], starts[s], 5)),
    ]
    for whole, device, part in pairs:
        first, second = part(slice(0, half)), part(slice(half, None))
        for w, d, p, q in zip(whole, device, first, second):
            assert host(d).tobytes() == w.tobytes()
            assert np.concatenate([p, q]).tobytes() == w.tobytes()
    d = c.dev.distance(ks, ks[::-1].copy())
    assert host(c.dev.distance_device(dev(ks), dev(ks[::-1].copy()))).tobytes() == d.tobytes()


def test_create_refuses_what_only_the_device_can_see(cases):
    from robopoker_amd import _lib
    from robopoker_amd.atlas import Atlas
    b = cases["b7"]
    obs, labels = torch.from_numpy(b.obs).to("cuda"), torch.from_numpy(b.labels).to("cuda")
    with pytest.raises(_lib.RpError, match="abstraction index >= K"):  # labels reach 6
        Atlas(1, obs, labels, 6, b.future[:6], b.weight[:6], below=cases["c"].dev)
    swapped = b.obs.copy()
    swapped[[10, 11]] = swapped[[11, 10]]
    with pytest.raises(_lib.RpError, match="IsomorphismIterator order"):
        Atlas(1, torch.from_numpy(swapped).to("cuda"), labels, 7, b.future, b.weight, below=cases["c"].dev)
    for below, future in ((cases["b256"].dev, b.future), (cases["river"].dev, b.future), (cases["c"].dev, b.future[:, :199])):
        with pytest.raises(_lib.RpError) as e:  # next of the same street, of street + 2, bins that are not next's K
            Atlas(1, obs, labels, 7, future, b.weight, below=below)
        assert e.value.code == _lib.RP_ERR_INVALID
    for call in (lambda: b.dev.neighbors([0], 0), lambda: b.dev.neighbors([0], 7), lambda: cases["c"].dev.neighbors([0], 17),
                 lambda: b.dev.members([0], [0], 0), lambda: b.dev.members([0], [0], 17),
                 lambda: _lib.check(_lib.load().rp_atlas_histograms(b.dev._h, 1, 2, b.labels.ctypes.data, b.labels.ctypes.data, b.labels.ctypes.data))):
        with pytest.raises(_lib.RpError) as e:
            call()
        assert e.value.code == _lib.RP_ERR_INVALID
    # a river atlas without the equity column, a street without a metric
    r = Atlas(3, torch.from_numpy(cases["river"].obs).to("cuda"), torch.from_numpy(cases["river"].labels).to("cuda"), 101)
    with pytest.raises(_lib.RpError) as e:
        r.obs_equity(cases["river"].obs[:4])
    assert e.value.code == _lib.RP_ERR_UNSUPPORTED
    for call in (lambda: r.neighbors([0], 1), lambda: r.distance([0], [1]), lambda: r.describe(cases["river"].obs[:1], [0]),
                 lambda: r.histograms("abs", [0])):
        with pytest.raises(_lib.RpError) as e:
            call()
        assert e.value.code == _lib.RP_ERR_UNSUPPORTED
    r.close()


def test_sinkhorn_cost_device_equals_the_host_form(gpu):
    from robopoker_amd import _lib, lloyd
    import ctypes as C
    rng = np.random.default_rng(9)
    bins, P = 24, 64
    tri = synthetic_tri(bins, 3) + F(0.125)
    mu, nu = rng.integers(0, 20, (P, bins)).astype(np.uint32), rng.integers(0, 20, (P, bins)).astype(np.uint32)
    mu[rng.random((P, bins)) < 0.4] = 0
    nu[3] = 0  # an empty side
    want, want_it = lloyd.sinkhorn_cost(mu, nu, tri)
    dmu, dnu = torch.from_numpy(mu.view(np.int32)).to("cuda"), torch.from_numpy(nu.view(np.int32)).to("cuda")
    out, it = torch.zeros(P, dtype=torch.float32, device="cuda"), torch.zeros(P, dtype=torch.int32, device="cuda")
    hp = lloyd.default_sinkhorn()
    for iterations in (it, None):
        out.zero_()
        _lib.check(_lib.load().rp_sinkhorn_cost_device(bins, P, dmu.data_ptr(), dnu.data_ptr(), tri.ctypes.data, C.byref(hp), 0, out.data_ptr(),
                                                       None if iterations is None else iterations.data_ptr()))
        assert out.cpu().numpy().tobytes() == want.tobytes()
    assert np.array_equal(it.cpu().numpy().view(np.uint32), want_it)


def test_obs_distance_composes_the_histograms_with_the_next_metric(cases):
    """Atlas.obs_distance / obs_abs_distance on (a) over (b)'s metric against the model's histograms under the CPU oracle's cost"""
    import oracle
    a, rng = cases["a"], random.Random(11)
    x = np.array([int(a.obs[rng.randrange(169)]) for _ in range(6)] + [0], np.int64)
    y = np.array([relabel(rng, int(a.obs[rng.randrange(169)])) for _ in range(6)] + [int(a.obs[0])], np.int64)
    ks = np.array([rng.randrange(169) for _ in range(7)], np.uint8)
    tri = cases["b256"].tri
    hx, sx = a.model.histograms(AM.HIST_OBS, x)
    for got, (hy, sy) in ((a.dev.obs_distance(x, y), a.model.histograms(AM.HIST_OBS, y)), (a.dev.obs_abs_distance(x, ks), a.model.histograms(AM.HIST_ABS, ks))):
        assert np.array_equal(got[1], np.maximum(sx, sy)) and got[1][-1] == AM.MISS
        for q in np.flatnonzero(got[1] == AM.OK):
            assert F(got[0][q]).tobytes() == F(oracle.sinkhorn_cost(hx[q], hy[q], tri)[0]).tobytes()
    with pytest.raises(ValueError, match="river"):
        cases["c"].dev.obs_distance(cases["c"].obs[:1], cases["c"].obs[:1])


def test_save_writes_the_two_tables(cases, tmp_path):
    from test_abi_atlas import read
    for name in ("b7", "river"):
        c = cases[name]
        paths = c.dev.save(str(tmp_path))
        rows, (a, s, p, e) = read(paths["abstraction"], "hhif", c.K)
        assert rows == c.K and np.array_equal(p.view(np.uint32), c.model.population) and e.tobytes() == c.model.equity.tobytes()
        assert (s == c.street).all() and a.tolist() == [c.street << 8 | k for k in range(c.K)]
        rows, (o, a, e, p) = read(paths["isomorphism"], "qhfi", c.obs.size)
        assert rows == c.obs.size and np.array_equal(o, c.obs) and np.array_equal(p.view(np.uint32), c.model.position)
        assert np.array_equal(a & 0xFF, c.labels)
        assert e.tobytes() == c.model.row_equity.tobytes() if c.street == 3 else (e.view(np.uint32) == 0xFFFFFFFF).all()

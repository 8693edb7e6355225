"""GPU: the reference's k-means++ draw (DefaultHasher(street) -> SmallRng, one WeightedIndex<f32> per pick) on a POINT-SHARDED layer:
rp_kmeans_kpp_ref_walk / _draw / _pick (csrc/kpp_refpick.hpp: the f32 running sum continued from the exact end sum of the shard
in front).  One device, handles playing the ranks, the floats handed on by hand.  Expected values: a host loop over the weights,
the oracle's single-process reference-seed k-means++ and a single lloyd.Layer in reference mode — everything bit for bit.
Also runs under RP_EMUL=1 RP_EMUL_GUARD=1 (logic only, small weight sets)."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
from lloyd_fixtures import flop_like_points, smooth_metric, turn_like_points
from robopoker_amd import _lib, lloyd
from test_gpu_lloyd import _host_weighted_index, _weight_sets

pytestmark = pytest.mark.gpu

V01 = (0.0, 0.37, 0.5, 0.9999999)


def _cuttings(n):
    """[0, n]; two ragged shards with an odd cut; four shards that include a 1-element shard and one shorter than a 256-chunk"""
    yield [0, n]
    if n >= 2:
        c = (n // 3) | 1
        yield [0, c if c < n else 1, n]
    if n >= 4:
        a = max(1, min(n - 3, (2 * n) // 5))
        b = a + 1                          # a 1-element shard
        c = min(n - 1, b + min(77, max(1, (n - b) // 2)))  # at most 77 elements: shorter than one chunk
        yield [0, a, b, c, n]


def _probe(w, cuts, v01):
    lib = _lib.load()
    cuts_a = np.asarray(cuts, dtype=np.uint64)
    out = np.zeros(3, dtype=np.uint64)
    ends = np.zeros(len(cuts) - 1, dtype=np.float32)
    rc = lib.rp_weighted_index_probe_shards(0, len(w), w.ctypes.data_as(C.c_void_p), len(cuts) - 1, cuts_a.ctypes.data_as(C.c_void_p),
                                            C.c_float(v01), out.ctypes.data_as(C.c_void_p), ends.ctypes.data_as(C.c_void_p))
    return rc, out, ends


def test_the_sharded_walk_equals_a_term_by_term_walk(gpu):
    big = os.environ.get("RP_EMUL") != "1"
    seen_small, seen_single = False, False
    for name, w in _weight_sets(big):
        cum = np.add.accumulate(w, dtype=np.float32)  # sequential
        for cuts in _cuttings(len(w)):
            assert all(b > a for a, b in zip(cuts, cuts[1:])) and cuts[0] == 0 and cuts[-1] == len(w), cuts
            if len(cuts) == 5:
                sizes = np.diff(cuts)
                seen_single |= bool((sizes == 1).any())
                seen_small |= bool(((sizes > 1) & (sizes < 256)).any()) or len(w) < 256
            want_ends = np.array([cum[c - 1] for c in cuts[1:]], dtype=np.float32)
            walked = None
            for v01 in V01:
                want_i, want_t = _host_weighted_index(w, v01)
                rc, out, ends = _probe(w, cuts, v01)
                if name == "all zero":
                    assert rc == _lib.RP_ERR_INVALID, (name, cuts, rc)
                    assert b"panics" in _lib.load().rp_last_error()
                else:
                    assert rc == 0, (name, cuts, v01, _lib.load().rp_last_error())
                assert int(out[0]) == want_i and int(out[1]) == int(np.float32(want_t).view(np.uint32)), (name, cuts, v01, list(out), want_i)
                assert np.array_equal(ends.view(np.uint32), want_ends.view(np.uint32)), (name, cuts, v01, ends, want_ends)
                walked = int(out[2])
            if name == "squared distances" and big:
                # the fast path is alive: of ~1172 chunks the single handle walks < 120 term by term (the first chunk, the binade
                # crossings, the ties); a shard with a prefix need not even walk its first chunk
                chunks = sum((b - a + 255) // 256 for a, b in zip(cuts, cuts[1:]))
                print(f"squared distances, {len(cuts) - 1} shard(s): {walked} of {chunks} chunks walked term by term")
                assert walked < chunks / 4, (cuts, walked, chunks)
    assert seen_single and seen_small


def _layers(kind, N, cuts, K=7, seed=4):
    if kind == "sinkhorn":
        bins, pts, tri = 32, flop_like_points(N, bins=32, mass=20, seed=seed), smooth_metric(32, seed)
    else:
        bins, pts, tri = 101, turn_like_points(N, bins=101, mass=46, seed=seed), None
    hp = oracle.default_sinkhorn()
    hp.iterations = 12
    shards = [lloyd.Layer(K, pts[a:b], kind, tri, hp=hp, seed=seed) for a, b in zip(cuts, cuts[1:])]
    single = oracle.OracleKmeans(K, pts, kind, tri, hp=hp, seed=seed)
    whole = lloyd.Layer(K, pts, kind, tri, hp=hp, seed=seed)
    counter = oracle.OracleKmeans(K, pts, kind, tri, hp=hp, seed=seed).init_centroids()  # the same layer's counter-draw picks
    return K, bins, shards, single, whole, counter


def _sharded_reference_picks(shards, cuts, K):
    """the protocol of rp_mi355x.h at rp_kmeans_set_rng, the ranks' floats handed on by hand"""
    for s in shards:
        s.kpp_begin()
    picks = []
    for k in range(K):
        ends, run = [], np.float32(0)
        for s in shards:
            run = s.kpp_ref_walk(run)
            assert isinstance(run, np.float32)
            ends.append(run)
        xs = [s.kpp_ref_draw(ends[-1]) for s in shards]
        assert all(x.view(np.uint32) == xs[0].view(np.uint32) for x in xs)  # every rank's generator in step
        owner = next(r for r in range(len(shards)) if ends[r] > xs[0])
        for r, s in enumerate(shards[:owner]):
            assert s.kpp_ref_pick(xs[0]) is None  # "not here": nothing written
        idx = shards[owner].kpp_ref_pick(xs[0])
        assert idx is not None
        hist = shards[owner].get_point(idx)
        picks.append(cuts[owner] + idx)
        for s in shards:
            s.set_centroid(k, hist)
            s.kpp_update(k)
    return np.array(picks, dtype=np.uint64)


@pytest.mark.parametrize("street", [1, 2])
@pytest.mark.parametrize("kind,N,cuts", [("sinkhorn", 300, [0, 131, 300]), ("sinkhorn", 300, [0, 77, 78, 300]),
                                         ("variation", 300, [0, 131, 300]), ("variation", 300, [0, 1, 189, 300]),
                                         ("variation", 2048, [0, 701, 1390, 2048])])
def test_sharded_reference_draw_on_one_gpu_matches_single(gpu, kind, N, cuts, street):
    import torch

    K, bins, shards, single, whole, counter = _layers(kind, N, cuts)
    W = len(shards)
    for s in shards:
        s.set_rng("reference", street)
    single.set_rng("reference", street)
    whole.set_rng("reference", street)
    picks = _sharded_reference_picks(shards, cuts, K)
    want = single.init_centroids()
    assert np.array_equal(picks, want), (picks, want)
    assert np.array_equal(picks, whole.init_centroids())
    assert not np.array_equal(picks, counter), "the reference draw gave the counter draw's picks: the mode is not live"
    for s in shards:
        s.init_bounds()
    single.init_bounds()
    nb = shards[0].partial_bytes()
    bufs = [torch.zeros(nb, dtype=torch.uint8, device="cuda") for _ in range(W)]
    words32 = K * bins + K
    off64 = (words32 * 4 + 7) & ~7
    for _ in range(3):
        for s, b in zip(shards, bufs):
            s.step_local(b.data_ptr())
        torch.cuda.synchronize()
        red = torch.zeros(nb, dtype=torch.uint8, device="cuda")
        red[: words32 * 4].view(torch.int32).copy_(sum(b[: words32 * 4].view(torch.int32) for b in bufs))
        red[off64:].view(torch.int64).copy_(sum(b[off64:].view(torch.int64) for b in bufs))
        torch.cuda.synchronize()
        outs = [s.step_finish(red.data_ptr()) for s in shards]
        d, sizes, _ = single.step()
        for od, osz, _ in outs:
            assert np.array_equal(od.view(np.uint32), d.view(np.uint32)) and np.array_equal(osz, sizes)
    sc, sw = single.centroids()
    sj, _, _ = single.bounds()
    for r, s in enumerate(shards):
        c, w = s.centroids()
        assert np.array_equal(c, sc) and np.array_equal(w, sw)
        j, _, _ = s.bounds()
        assert np.array_equal(j, sj[cuts[r]:cuts[r + 1]])


def test_misuse_is_refused_and_the_handle_stays_usable(gpu):
    K, bins, shards, _, _, _ = _layers("variation", 300, [0, 131, 300])
    lib = _lib.load()
    s = shards[0]
    s.kpp_begin()
    with pytest.raises(_lib.RpError) as e:  # counter mode
        s.kpp_ref_walk(np.float32(0))
    assert "rp_kmeans_set_rng" in str(e.value)
    s.set_rng("reference", 1)
    with pytest.raises(_lib.RpError) as e:  # reference mode, generator not seeded
        s.kpp_ref_walk(np.float32(0))
    assert "rp_kmeans_kpp_begin" in str(e.value)
    s.kpp_begin()
    with pytest.raises(_lib.RpError) as e:  # no walk yet
        s.kpp_ref_pick(np.float32(0.5))
    assert "rp_kmeans_kpp_ref_walk" in str(e.value)
    with pytest.raises(_lib.RpError) as e:
        s.kpp_ref_draw(np.float32(0))
    assert "panics" in str(e.value)
    assert lib.rp_last_error()
    # still usable: the handle plays a whole layer of its own (one shard, prefix 0) against a single layer over the same points
    end = s.kpp_ref_walk(np.float32(0))
    assert end == np.float32(131)  # potentials are all 1 after kpp_begin
    pts_picks = _sharded_reference_picks([s], [0, 131], K)  # kpp_begin seeds the generator again
    ref = lloyd.Layer(K, turn_like_points(300, bins=101, mass=46, seed=4)[:131], "variation", None, seed=4)
    ref.set_rng("reference", 1)
    assert np.array_equal(pts_picks, ref.init_centroids())

"""ShardedLayer(rng="reference") with a world of TWO and of THREE — on a machine without a GPU.  The reference's k-means++ draw
(DefaultHasher(street) -> SmallRng, one WeightedIndex<f32> per pick) runs its f32 running sum from rank to rank: one float handed
on per rank per pick (dist.send / recv over gloo), the total and the end sums all-gathered, the pick on the first rank whose end
sum exceeds the draw.  Every rank loads the kernels' sources under the wave64 execution model (tests/emul) over its
own ragged shard.  Expected values: the oracle's single-process reference-seed k-means++ and Elkan steps, bit for bit."""
from __future__ import annotations

import multiprocessing as mp
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "emul")
CLANG = os.environ.get("RP_EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")
N = 200
CUTS = {2: [0, 117, N], 3: [0, 61, 117, N]}  # ragged shards; with three ranks the sum passes through a middle rank


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _enter(rank, port, world):
    """in a rank process: gloo (the hand-offs, the collectives and the comparisons), then the emulated library"""
    for p in (ROOT, os.path.join(ROOT, "tests"), EMUL):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import harness

    harness.load_emulated(build=False)
    return dist


def _gather_to_zero(dist, arr, rank, world, nbytes):
    """rank 0 receives every rank's array as bytes (nbytes[r] known to it), in rank order"""
    import torch

    mine = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy())
    if rank:
        dist.send(mine, dst=0)
        return None
    parts = [mine.numpy()]
    for r in range(1, world):
        other = torch.zeros(nbytes[r], dtype=torch.uint8)
        dist.recv(other, src=r)
        parts.append(other.numpy())
    return parts


def _kmeans_refdraw(rank, port, out, kind, world):
    dist = _enter(rank, port, world)
    import torch

    import oracle
    from lloyd_fixtures import smooth_metric, turn_like_points
    from robopoker_amd import lloyd
    from robopoker_amd.parallel import ShardedLayer

    K, bins, mass, seed, street = 6, (24 if kind == "sinkhorn" else 101), (14 if kind == "sinkhorn" else 46), 9, 1
    pts = turn_like_points(N, bins=bins, mass=mass, seed=seed)
    tri = smooth_metric(bins, seed) if kind == "sinkhorn" else None
    hp = oracle.default_sinkhorn()
    hp.iterations = 12
    cuts = CUTS[world]
    lo, hi = cuts[rank], cuts[rank + 1]
    eng = lloyd.Layer(K, pts[lo:hi], kind, tri, hp=hp, seed=seed)
    sh = ShardedLayer(eng, K, bins, seed, device="cpu", rng="reference", street=street)
    chosen = sh.init_centroids()
    # (owner, local index on the owner | None): every rank names the same owners; the owner's index -> the global one
    owners = np.array([o for o, _ in chosen], dtype=np.int64)
    mine = np.array([cuts[o] + i if o == rank else -1 for o, i in chosen], dtype=np.int64)
    assert all((i is not None) == (o == rank) for o, i in chosen)
    t = torch.from_numpy(mine.copy())
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    picks = t.numpy().astype(np.uint64)
    c0, w0 = eng.centroids()
    sh.init_bounds()
    drifts, sizes = [], None
    for _ in range(3):
        d, sizes, _ = sh.step()
        drifts.append(np.array(d, copy=True))
    c, w = eng.centroids()
    j, _, _ = eng.bounds()
    shard_sizes = [b - a for a, b in zip(cuts, cuts[1:])]
    all_j = _gather_to_zero(dist, j, rank, world, [n * j.itemsize for n in shard_sizes])
    all_owner = _gather_to_zero(dist, owners, rank, world, [owners.nbytes] * world)
    all_c0 = _gather_to_zero(dist, c0, rank, world, [c0.nbytes] * world)
    all_c = _gather_to_zero(dist, c, rank, world, [c.nbytes] * world)
    ok = True
    if rank == 0:
        single = oracle.OracleKmeans(K, pts, kind, tri, hp=hp, seed=seed)
        counter = oracle.OracleKmeans(K, pts, kind, tri, hp=hp, seed=seed).init_centroids()
        single.set_rng("reference", street)
        want = single.init_centroids()
        sc0, _ = single.centroids()
        single.init_bounds()
        sd, ssz = [], None
        for _ in range(3):
            d, ssz, _ = single.step()
            sd.append(d.copy())
        sc, sw = single.centroids()
        sj, _, _ = single.bounds()
        checks = {
            "picks": np.array_equal(picks, want),
            "not the counter draw": not np.array_equal(picks, counter),
            "owners agree": all(np.array_equal(o, all_owner[0]) for o in all_owner),
            "centroids after k-means++": all(np.array_equal(a, np.ascontiguousarray(sc0).view(np.uint8).reshape(-1)) for a in all_c0),
            "centroids identical on all ranks": all(np.array_equal(a, all_c[0]) for a in all_c),
            "centroids": np.array_equal(c, sc) and np.array_equal(w, sw),
            "sizes": np.array_equal(sizes, ssz),
            "drift": all(np.array_equal(np.asarray(a).view(np.uint32), b.view(np.uint32)) for a, b in zip(drifts, sd)),
            "assignments": np.array_equal(np.concatenate(all_j), np.ascontiguousarray(sj).view(np.uint8).reshape(-1)),
        }
        ok = all(checks.values())
        if not ok:
            print("sharded reference draw:", checks, picks, want, file=sys.stderr, flush=True)
    out.put((f"refdraw-{rank}", bool(ok)))
    dist.barrier()
    dist.destroy_process_group()


def _guarded(fn, rank, port, out, *args):
    """a rank that raises still reports (the parent would otherwise wait for its timeout)"""
    try:
        fn(rank, port, out, *args)
    except BaseException as exc:  # noqa: BLE001
        import traceback

        traceback.print_exc()
        out.put((f"error-{rank}", f"{type(exc).__name__}: {exc}"))
        raise


@pytest.fixture(scope="module")
def emul_lib():
    if not os.path.exists(CLANG):
        pytest.skip(f"{CLANG} (host compiler of the execution model) is not installed")
    sys.path.insert(0, EMUL)
    import build as emul_build

    emul_build.build(jobs=os.cpu_count() or 4)
    return emul_build.LIB


def _run(fn, *args, world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    saved = os.environ.get("RP_EMUL_THREADS")
    os.environ["RP_EMUL_THREADS"] = str(max(1, 8 // world))  # the ranks share the host's cores
    try:
        procs = [ctx.Process(target=_guarded, args=(fn, r, port, q) + args) for r in range(world)]
        for p in procs:
            p.start()
    finally:
        if saved is None:
            os.environ.pop("RP_EMUL_THREADS", None)
        else:
            os.environ["RP_EMUL_THREADS"] = saved
    results = dict(q.get(timeout=600) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    assert not [k for k in results if k.startswith("error")], results
    assert all(p.exitcode == 0 for p in procs)
    return results


@pytest.mark.parametrize("kind,world", [("sinkhorn", 2), ("variation", 2), ("variation", 3)])
def test_sharded_reference_draw_equals_single_process(emul_lib, kind, world):
    assert _run(_kmeans_refdraw, kind, world, world=world) == {f"refdraw-{r}": True for r in range(world)}


def test_the_counter_draw_stays_the_default():
    # the constructor's new keywords change nothing unless asked for (bench.py constructs ShardedLayer without them)
    import inspect

    from robopoker_amd.parallel import ShardedLayer
    from robopoker_amd.pretraining import cluster_layer_sharded, run_sharded

    p = inspect.signature(ShardedLayer.__init__).parameters
    assert p["rng"].default == "counter" and p["street"].default == 1
    for fn in (cluster_layer_sharded, run_sharded):
        q = inspect.signature(fn).parameters
        assert q["libm"].default == "contract" and q["rng"].default == "counter"

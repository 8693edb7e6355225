#!/usr/bin/env python3
"""What the rank-to-rank chain of the sharded reference-seed k-means++ draw costs in launches and synchronisations.
ONE device, W handles over contiguous shards of the same flop-size point set, the f32 running sum handed on in process:
    per pick:  handle 0 .. W-1: kpp_ref_walk(prefix) -> end sum;  every handle: kpp_ref_draw(total);  the owner: kpp_ref_pick(x)
Only walk + draw + pick are timed (no kpp_update).  The first `--prelude` picks run the whole protocol with set_centroid + kpp_update
(untimed) so that the potentials are squared distances, and are compared with a single layer's picks; from then on the potentials
only lose the picked points.  Next to it: the single layer's fused draw (rp_kmeans_init_centroids, the "ref_draw" clock: HIP events).
There is one device per machine, so no time of a true W-rank run exists: the figures are labelled for what they are.

    python scripts/sharded_refdraw_timing.py [--n 1286792] [--k 256] [--worlds 1,2,8] [--prelude 8] [--points pts.npy] [--out file.json]
"""
import argparse
import json
import os
import signal
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np  # noqa: E402

from robopoker_amd import lloyd  # noqa: E402
from robopoker_amd.fixtures import flop_like_points, smooth_metric  # noqa: E402

BINS, STREET = 256, 1


def chain(handles, cuts):
    """one pick of the protocol (rp_mi355x.h at rp_kmeans_set_rng); returns (owner, local index, global index)"""
    ends, run = [], np.float32(0)
    for h in handles:
        run = h.kpp_ref_walk(run)
        ends.append(run)
    x = None
    for h in handles:
        x = h.kpp_ref_draw(ends[-1])
    owner = next(r for r in range(len(handles)) if ends[r] > x)
    idx = handles[owner].kpp_ref_pick(x)
    return owner, idx, cuts[owner] + idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1286792)
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--worlds", default="1,2,8")
    ap.add_argument("--prelude", type=int, default=8)
    ap.add_argument("--points", default=None, help=".npy of (n, 256) u8 histograms; generated from the bench's seed when absent")
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=900, help="seconds after which the script ends itself")
    a = ap.parse_args()
    K = a.k
    signal.alarm(a.timeout)
    pts = np.load(a.points) if a.points else flop_like_points(a.n, bins=BINS, mass=47, seed=0xF10F)
    pts = np.ascontiguousarray(pts[: a.n])
    n = pts.shape[0]
    tri = smooth_metric(BINS, 1)
    res = {"N": n, "K": K, "prelude_picks": a.prelude,
           "label": "one device, W handles: launch + sync overhead of the chain, no interconnect", "worlds": {}}
    single = lloyd.Layer(K, pts, "sinkhorn", tri, seed=1)
    single.set_rng("reference", STREET)
    single.profile(True)
    t0 = time.perf_counter()
    want = single.init_centroids()
    wall = time.perf_counter() - t0
    ms, launches = single.kernel_time("ref_draw")
    st = single.prune_stats()
    res["single_fused"] = {"draw_ms_per_pick_events": ms / K, "draw_s_per_layer_events": ms * 1e-3, "launch_groups": launches,
                           "kmeanspp_wall_s": wall, "chunks": st.get("ref_pick_chunks"), "walked_term_by_term": st.get("ref_pick_walked"),
                           "note": "rp_kmeans_init_centroids: summaries + fused walk/draw/pick, potentials updated after every pick"}
    single.close()
    print(json.dumps({"single_fused": res["single_fused"]}), flush=True)
    for W in [int(w) for w in a.worlds.split(",")]:
        width = (n + W - 1) // W
        cuts = [min(n, r * width) for r in range(W + 1)]
        hs = [lloyd.Layer(K, pts[cuts[r]:cuts[r + 1]], "sinkhorn", tri, seed=1) for r in range(W)]
        for h in hs:
            h.set_rng("reference", STREET)
            h.profile(True)
            h.kpp_begin()
        picks = []
        for k in range(a.prelude):
            owner, idx, g = chain(hs, cuts)
            picks.append(g)
            hist = hs[owner].get_point(idx)
            for h in hs:
                h.set_centroid(k, hist)
                h.kpp_update(k)
        ev0 = sum(h.kernel_time("ref_draw")[0] for h in hs)
        t0 = time.perf_counter()
        for k in range(a.prelude, K):
            chain(hs, cuts)
        wall = time.perf_counter() - t0
        ev = sum(h.kernel_time("ref_draw")[0] for h in hs) - ev0
        timed = K - a.prelude
        walked = sum(h.prune_stats().get("ref_pick_walked", 0) for h in hs)
        chunks = sum(h.prune_stats().get("ref_pick_chunks", 0) for h in hs)
        res["worlds"][str(W)] = {"ms_per_pick_wall": wall * 1e3 / timed, "ms_per_pick_events_all_handles": ev / timed,
                                 "timed_picks": timed, "prelude_picks_equal_single": bool(np.array_equal(picks, want[: a.prelude])),
                                 "chunks": chunks, "walked_term_by_term": walked}
        for h in hs:
            h.close()
        print(json.dumps({str(W): res["worlds"][str(W)]}), flush=True)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
    return 0 if all(w["prelude_picks_equal_single"] for w in res["worlds"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())

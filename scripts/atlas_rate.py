#!/usr/bin/env python3
"""Time of the abstraction atlas (rp_atlas, csrc/atlas.hip) at full size, against the same tables derived on the same device by torch.

Tables: the whole flop, turn and river isomorphism lists.  The river's labels are rp_river_equity's buckets (K = 101); the flop and
the turn get stand-in labels (a hash of the observation into K = 128 / 200: clustering is not what is measured) with synthetic
centroids and metric.

  create   rp_atlas_create, a warm-up and then --runs creates; the library's own HIP events split each into the (abs, obs) sort and
           the rest (histogram, scan, positions, equity): rp_atlas_create_ms.  Median, min, max.
  bytes    what the sort built has to move, from its shape: per round of at most 27 key bits the digit kernel reads obs + abs (9 B a
           row; 4 B more for the permutation in the second round) and writes the digit (and the row index in the first round); per
           radix pass the histogram reads 4 B a row, the scatter reads 8 B and writes 8 B.  Over the sort's time, as a fraction of 8 TB/s.
  torch    the yardstick: a stable argsort of abs << 54 | obs, a bincount, a cumsum and a scatter for the positions, timed by
           torch.cuda.Event after a warm-up.  ratio = torch / atlas create (sort + rest; the rest holds the atlas' equity kernel, which
           the yardstick has no counterpart of, and the sort's interval the allocation of its temporaries).
  queries  2^20 queries of each kind through the _device forms (which return after the device finished), host clock, on the turn
           atlas (describe and pick on the river too).

    atlas_rate.py [--streets flop,turn,rive] [--runs 3] [--queries 1048576] [--pockets 1326] [--out profiles/atlas_rate.json]
"""
import argparse
import json
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
say = lambda m: print(m, file=sys.stderr, flush=True)  # noqa: E731
HBM_BYTES_PER_S = 8e12
N_CARDS = {"flop": 5, "turn": 6, "rive": 7}
STAND_IN_K = {"flop": 128, "turn": 200}


def sort_shape(n_cards):
    """(rounds of key bits, radix passes per round) as csrc/atlas.hip and sortscan.hpp's sort_pairs choose them"""
    total = 6 * n_cards + 8
    rounds = [min(total, 27)] + ([total - 27] if total > 27 else [])
    passes = [(b + 8) // 9 if 24 < b <= 27 else (b + 7) // 8 for b in rounds]
    return rounds, passes


def sort_bytes(n, n_cards):
    rounds, passes = sort_shape(n_cards)
    digits = (9 + 4 + 4) + ((9 + 4 + 4) if len(rounds) > 1 else 0)
    return n * (digits + 20 * sum(passes))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streets", default="flop,turn,rive")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--pockets", type=int, default=1326, help="only the first POCKETS pockets of every list (a rehearsal; the default is all)")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "atlas_rate.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from robopoker_amd import deuce
    from robopoker_amd.atlas import Atlas

    if not torch.cuda.is_available():
        raise SystemExit("atlas_rate.py measures on the GPU: no device visible")
    rng = np.random.default_rng(2026)
    out = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "hbm_bytes_per_s": HBM_BYTES_PER_S,
           "timing": "create: HIP events inside the library (rp_atlas_create_ms); torch: torch.cuda.Event; queries: host clock around "
                     "_device calls that end in a device synchronise; a warm-up, then the runs; median / min / max",
           "streets": {}, "queries": {}}

    def stats(ts):
        return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}

    def torch_tables(obs, labels, K):
        key = (labels.to(torch.int64) << 54) | obs
        members = torch.argsort(key, stable=True)
        population = torch.bincount(labels.to(torch.int64), minlength=K)
        offset = torch.cumsum(population, 0) - population
        position = torch.empty_like(members)
        position[members] = torch.arange(members.numel(), device=obs.device) - offset[labels[members].to(torch.int64)]
        return members, population, position

    atlases = {}
    below = None
    for street in ("rive", "turn", "flop"):
        if street not in args.streets.split(","):
            continue
        obs = deuce.isomorphisms(street, 0, args.pockets)
        n = obs.numel()
        if street == "rive":
            eq, labels = deuce.river_equity(obs)
            K, kw = 101, dict(row_equity=eq)
        else:
            K = STAND_IN_K[street]
            labels = (((obs * 2654435761) >> 20) % K).to(torch.uint8)
            bins = below.K if below is not None else 101
            if below is None:  # the street above alone: a one-row stand-in chain below it is not worth a river list
                raise SystemExit("--streets must hold every street below the ones asked for")
            future = rng.integers(0, 40, (K, bins)).astype(np.uint32)
            kw = dict(future=future, future_weight=future.sum(axis=1).astype(np.uint64),
                      metric=rng.random(K * (K - 1) // 2).astype(np.float32), below=below)
        sort_ms, rest_ms = [], []
        a = None
        for run in range(args.runs + 1):
            if a is not None:
                a.close()
            a = Atlas(street, obs, labels, K, **kw)
            if run:
                s, r = a.create_ms()
                sort_ms.append(s)
                rest_ms.append(r)
        yard = []
        for run in range(args.runs + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            members, population, position = torch_tables(obs, labels, K)
            e1.record()
            torch.cuda.synchronize()
            if run:
                yard.append(e0.elapsed_time(e1))
        t = a.tables_device()
        assert torch.equal(t["members"].to(torch.int64), members) and torch.equal(t["position"].to(torch.int64), position)
        assert torch.equal(t["population"].to(torch.int64), population)
        del members, population, position, t
        rounds, passes = sort_shape(N_CARDS[street])
        nbytes = sort_bytes(n, N_CARDS[street])
        total = [s + r for s, r in zip(sort_ms, rest_ms)]
        res = {"rows": n, "K": K, "sort": stats(sort_ms), "rest": stats(rest_ms), "create": stats(total), "key_bits": 6 * N_CARDS[street] + 8,
               "rounds_of_key_bits": rounds, "radix_passes": passes, "sort_bytes": nbytes,
               "sort_bytes_per_s": nbytes / (np.median(sort_ms) * 1e-3), "sort_fraction_of_hbm": nbytes / (np.median(sort_ms) * 1e-3) / HBM_BYTES_PER_S,
               "sort_ms_per_pass": float(np.median(sort_ms)) / sum(passes), "torch": stats(yard),
               "torch_over_atlas": float(np.median(yard) / np.median(total)), "tables_equal_torch": True}
        say(f"{street}: {n} rows, sort {res['sort']['median_ms']:.2f} ms ({sum(passes)} passes, {res['sort_fraction_of_hbm'] * 100:.1f} % of 8 TB/s), "
            f"rest {res['rest']['median_ms']:.2f} ms, torch {res['torch']['median_ms']:.2f} ms: torch / atlas = {res['torch_over_atlas']:.2f}")
        out["streets"][street] = res
        atlases[street] = (a, obs)
        below = a

    Q = args.queries
    dev = torch.device("cuda", 0)

    def timed(fn):
        fn()
        ts = []
        for _ in range(args.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {**stats(ts), "queries_per_s": Q / (float(np.median(ts)) * 1e-3)}

    for street in ("turn", "rive"):
        if street not in atlases:
            continue
        a, obs = atlases[street]
        rows = torch.randint(0, obs.numel(), (Q,), device=dev)
        q_obs = obs[rows].contiguous()
        ks = torch.randint(0, a.K, (Q,), device=dev).to(torch.uint8)
        draw = torch.randint(-(1 << 62), 1 << 62, (Q,), device=dev, dtype=torch.int64)
        res = {"describe": timed(lambda: a.describe_device(q_obs)), "pick": timed(lambda: a.pick_device(ks, draw)),
               "obs_equity": timed(lambda: a.obs_equity_device(q_obs)),
               "members_6": timed(lambda: a.members_device(ks, torch.zeros(Q, dtype=torch.int32, device=dev), 6))}
        if street == "turn":
            draws = torch.randint(-(1 << 62), 1 << 62, (Q, 6), device=dev, dtype=torch.int64)
            res.update({"describe_wrt": timed(lambda: a.describe_device(q_obs, ks)), "neighbors_6": timed(lambda: a.neighbors_device(ks, 6)),
                        "neighbors_6_with_draws": timed(lambda: a.neighbors_device(ks, 6, False, draws)),
                        "distance": timed(lambda: a.distance_device(ks, ks.flip(0).contiguous())),
                        "histograms_abs": timed(lambda: a.histograms_device("abs", ks)), "histograms_obs": timed(lambda: a.histograms_device("obs", q_obs))})
        for k, v in res.items():
            say(f"{street} {k}: {v['median_ms']:.3f} ms for {Q} queries = {v['queries_per_s'] / 1e6:.1f} M/s")
        out["queries"][street] = res
    out["queries_note"] = "each time includes the output tensors' allocation and zeroing by the Python face"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps({s: {"sort_ms": r["sort"]["median_ms"], "rest_ms": r["rest"]["median_ms"], "torch_ms": r["torch"]["median_ms"],
                          "torch_over_atlas": r["torch_over_atlas"]} for s, r in out["streets"].items()}))


if __name__ == "__main__":
    main()

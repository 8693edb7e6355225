#!/usr/bin/env python3
"""Rate of the subgame-world query (rp_nlhe_restrict, csrc/nlmc_world.hpp) against the range query it is built on, and against the
route a caller had before it existed.

Workload: river recalls — a 15-edge history (three streets checked through, a raising war on the river), 990 candidate holes and 6
subject nodes each — at batches 1, 64 and 4 096, with `deals` 1 (the reference's use: one opponent hole per solver iteration) and 64,
every world drawn from the belief's weights.  64 distinct recalls (boards and holes drawn from a seed); larger batches repeat them,
each with deal ids of its own.  The table is a blueprint trained for `--train-steps` steps of `--train-batch` trees with the hash
encoder.

  restrict    rp_nlhe_restrict_device: the recalls already in device memory, one launch (replay, reaches, bucket masses, partition,
              deals), timed from the call to rp_nlhe_sync.
  range       rp_nlhe_opponent_range_device on the same recalls, timed the same way: the floor the new kernel sits on (its phases A - C).
  host_route  what the parent commit offers for the same answer: the rp_nlhe_opponent_range HOST form — recalls up, mass / seen back.
              The partition and the rejection sampler the caller would then run on the host are NOT in the timed window (here they are
              the test model in Python, timed on their own): the figure is a lower bound of that route.
All three are timed with a host clock, alternating, `--runs` runs each after a warm-up of every shape; median, min and max.
The answers are compared bit for bit at every batch: world / weights of rp_nlhe_belief_device against the model's partition of the
host route's mass / seen for every recall, and holes / world / attempts of every deal against the model's sequential sampler (which
buckets each attempted hole with the oracle) — every recall at batches up to 64, the first and the last 64 recalls beyond.

    nlhe_world_rate.py [--cap-log2 20] [--runs 5] [--batches 1,64,4096] [--deals 1,64] [--out profiles/nlhe_world_rate.json]
"""
import argparse
import json
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
say = lambda m: print(m, file=sys.stderr, flush=True)  # noqa: E731

# as hipcc -Rpass-analysis=kernel-resource-usage reports them for gfx950 (csrc/Makefile's flags)
STATIC = {"k_nl_world": {"vgprs": 57, "agprs": 0, "sgprs": 106, "sgpr_spills": 72, "vgpr_spills": 0, "scratch_bytes_per_lane": 0,
                         "lds_bytes_per_block": 10528, "occupancy_waves_per_simd": 7, "block": 256},
          "k_nl_partition": {"vgprs": 20, "agprs": 0, "sgprs": 57, "sgpr_spills": 0, "vgpr_spills": 0, "scratch_bytes_per_lane": 0,
                             "lds_bytes_per_block": 2608, "occupancy_waves_per_simd": 8, "block": 256},
          "k_nl_range": {"vgprs": 60, "agprs": 0, "sgprs": 106, "sgpr_spills": 71, "vgpr_spills": 0, "scratch_bytes_per_lane": 0,
                         "lds_bytes_per_block": 7920, "occupancy_waves_per_simd": 7, "block": 256}}
SEED = 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cap-log2", type=int, default=20)
    ap.add_argument("--train-steps", type=int, default=4)
    ap.add_argument("--train-batch", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--batches", default="1,64,4096")
    ap.add_argument("--deals", default="1,64")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "nlhe_world_rate.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import nlhe_world_model as WM
    import oracle_nlhe as ON
    from robopoker_amd.nlhe import NlheSolver, Recall

    if not torch.cuda.is_available():
        raise SystemExit("nlhe_world_rate.py measures on the GPU: no device visible")
    rng = np.random.default_rng(2026)
    pot = ON.RaiseOdds(1, 1)
    edges = [ON.Open(2), pot, ON.E_CALL, 1, 3, 3, 1, 3, 3, 1, 3, pot, pot, pot, ON.E_CALL]
    recalls = []
    for _ in range(args.distinct):
        c = [int(x) for x in rng.permutation(52)[:7]]
        recalls.append(Recall(0, 1 << c[0] | 1 << c[1], [1 << c[2] | 1 << c[3] | 1 << c[4], 1 << c[5], 1 << c[6]], edges))

    s = NlheSolver(cap_log2=args.cap_log2, batch=args.train_batch, seed=1)
    for _ in range(args.train_steps):
        s.step("composed")
    keys = s.counters()[2]
    say(f"table: 2^{args.cap_log2} rows, {keys} infosets after {args.train_steps} steps of {args.train_batch} trees")

    # ---- the host side of the parent's route for the distinct recalls: the model's partition of the host form's mass / seen
    mass, seen, status = s.opponent_range(recalls)
    assert not status.any(), "a recall of the workload was refused"
    t0 = time.perf_counter()
    beliefs = []
    for i in range(args.distinct):
        world, weights, total = WM.partition(mass[i], seen[i])
        beliefs.append(dict(status=0, world=world, weights=weights, total=total))
    partition_s = time.perf_counter() - t0
    caches = [{} for _ in recalls]
    sampler = {"deals": 0, "seconds": 0.0, "attempts": 0}

    def model_deals(i, r, deals):
        """recall r of a batch (the distinct recall i) -> the model's (holes, world, attempts) of its deals, worlds drawn"""
        t0 = time.perf_counter()
        out = [WM.restrict_one(recalls[i], beliefs[i], WM.WORLD_NONE, WM.Deal(SEED, WM.deal_id(0, r, deals, d)), cache=caches[i]) for d in range(deals)]
        sampler["seconds"] += time.perf_counter() - t0
        sampler["deals"] += deals
        sampler["attempts"] += sum(o[2] for o in out)
        return out

    out = {"device": torch.cuda.get_device_name(0), "cap_log2": args.cap_log2, "infosets": int(keys), "train_steps": args.train_steps,
           "train_batch": args.train_batch, "distinct_recalls": args.distinct, "holes_per_recall": 990, "runs": args.runs,
           "static_resources": STATIC,
           "timing": "host clock; restrict and range: _device forms, from the call to rp_nlhe_sync; host_route: the rp_nlhe_opponent_range host "
                     "form (it synchronises); alternating; median / min / max of the runs",
           "results": {}}
    all_equal = True
    for n in [int(b) for b in args.batches.split(",")]:
        idx = np.arange(n) % args.distinct
        rec_host = Recall.pack([recalls[i] for i in idx])
        rec = torch.from_numpy(rec_host.view(np.uint8).copy()).to("cuda")
        check = sorted(set(range(min(n, 64))) | set(range(max(0, n - 64), n)))
        # the belief of every recall of the batch against the model's partition
        bel = s.belief_device(rec)
        s.sync()
        same = bool(not bel["status"].cpu().numpy().any()
                    and np.array_equal(bel["world"].cpu().numpy(), np.stack([beliefs[i]["world"] for i in idx]))
                    and np.array_equal(bel["weights"].cpu().numpy().view(np.uint32), np.stack([beliefs[i]["weights"] for i in idx]).view(np.uint32)))
        res = {}
        for deals in [int(d) for d in args.deals.split(",")]:
            def restrict():
                t0 = time.perf_counter()
                ans = s.restrict_device(rec, deals, None, SEED, 0)
                s.sync()
                return time.perf_counter() - t0, ans

            def floor():
                t0 = time.perf_counter()
                ans = s.opponent_range_device(rec)
                s.sync()
                return time.perf_counter() - t0, ans

            def host_route():
                t0 = time.perf_counter()
                ans = s.opponent_range(rec_host)
                return time.perf_counter() - t0, ans

            _, got = restrict()  # warm-up of every shape, and the comparison of the answers
            floor()
            host_route()
            holes, world, attempts = (got[f].cpu().numpy() for f in ("holes", "world", "attempts"))
            deals_same = not got["status"].cpu().numpy().any()
            for r in check:
                want = model_deals(int(idx[r]), r, deals)
                deals_same = deals_same and all((int(holes[r, d]), int(world[r, d]), int(attempts[r, d]) & 0xFFFF) == want[d] for d in range(deals))
            tr, tf, th = [], [], []
            for _ in range(args.runs):
                tr.append(restrict()[0])
                tf.append(floor()[0])
                th.append(host_route()[0])
            entry = {"model_bits_equal": bool(deals_same), "recalls_compared": len(check), "mean_attempts": float(attempts.astype(np.uint16).mean()),
                     "fallbacks": int((attempts.astype(np.uint16) == WM.MAX_REJECTIONS).sum())}
            for name, ts in (("restrict", tr), ("range", tf), ("host_route_lower_bound", th)):
                med = float(np.median(ts))
                entry[name] = {"seconds": ts, "median_s": med, "min_s": min(ts), "max_s": max(ts), "recalls_per_s": n / med}
            entry["restrict"]["deals_per_s"] = n * deals / entry["restrict"]["median_s"]
            entry["restrict_over_range"] = entry["restrict"]["median_s"] / entry["range"]["median_s"]
            entry["host_route_over_restrict"] = entry["host_route_lower_bound"]["median_s"] / entry["restrict"]["median_s"]
            entry["bytes_moved"] = {"restrict_back_if_copied": n * deals * 11 + n, "host_route_up": n * 88, "host_route_back": n * (256 * 5 + 1)}
            same = same and deals_same
            res[f"deals_{deals}"] = entry
            say(f"batch {n}, deals {deals}: restrict {entry['restrict']['median_s'] * 1e3:.3f} ms [{min(tr) * 1e3:.3f}, {max(tr) * 1e3:.3f}], range "
                f"{entry['range']['median_s'] * 1e3:.3f} ms [{min(tf) * 1e3:.3f}, {max(tf) * 1e3:.3f}], host route >= "
                f"{entry['host_route_lower_bound']['median_s'] * 1e3:.3f} ms [{min(th) * 1e3:.3f}, {max(th) * 1e3:.3f}]; mean attempts "
                f"{entry['mean_attempts']:.2f}; same bits: {deals_same}")
        res["belief_bits_equal"] = same
        all_equal = all_equal and same
        out["results"][str(n)] = res
    out["model_bits_equal"] = bool(all_equal)
    out["host_side_of_the_parents_route"] = {
        "partition_seconds_for_the_distinct_recalls": partition_s, "sampler_seconds": sampler["seconds"], "sampler_deals": sampler["deals"],
        "sampler_attempts": sampler["attempts"],
        "how": "tests/nlhe_world_model.py in Python: the partition over np.float32 scalars, the sampler bucketing each attempted hole with "
               "the CPU oracle's isomorphism (memoised per hole); not in any timed window above"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps({"model_bits_equal": out["model_bits_equal"],
                      **{f"{b}x{d}": {"restrict_ms": e["restrict"]["median_s"] * 1e3, "restrict_over_range": e["restrict_over_range"],
                                      "host_route_over_restrict": e["host_route_over_restrict"]}
                         for b, r in out["results"].items() for d, e in r.items() if d.startswith("deals_")}}))


if __name__ == "__main__":
    main()

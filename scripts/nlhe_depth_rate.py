#!/usr/bin/env python3
"""Rate of the depth-limited re-solve (rp_nlhe_depth_solve, csrc/nlmc_depth.hpp) against the frontier-payoff query it is built on, and
against the route a caller had before it existed.

Workload: flop entries — open, call, the flop, seat 0 to act — with origin = street - 1 (the 4 x 4 continuation game at the turn
boundary), rollouts = 16, at batches 1, 64 and 4 096 and `--iterations` (64 and 8).  64 distinct entries (holes and flops drawn from a
seed); larger batches repeat them, each with an id of its own.  The table is a blueprint trained for `--train-steps` steps of
`--train-batch` trees with the hash encoder.

  solve       rp_nlhe_depth_solve_device: the entries already in device memory, one launch, timed from the call to rp_nlhe_sync.
              Solves that end with a status (a local profile or a tree that outgrew its region) are counted and do not enter the
              iterations / rollouts rates.
  frontier    rp_nlhe_frontier_payoffs_device on as many frontiers as the solves of that batch played in all (the chance state after
              check, check of the same entries), one launch, timed the same way: the floor the solver sits on.
  host_route  the parent commit's route for ONE solve, as a lower bound: per iteration one rp_nlhe_frontier_payoffs_device launch on
              the mean number of frontiers of a tree and one rp_nlhe_sync; the tree, the regret matching and the local profile the
              caller would run on the host between them are NOT in the timed window.
All are timed with a host clock, alternating, `--runs` runs each after a warm-up of every shape; median, min and max.
`model_bits_equal`: the first entries solved for 2 iterations against tests/nlhe_depth_model.py over the exported table, result and rows.

    nlhe_depth_rate.py [--cap-log2 20] [--runs 5] [--batches 1,64,4096] [--iterations 64,8] [--out profiles/nlhe_depth_rate.json]
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
STATIC = {"k_nl_depth": {"vgprs": 146, "agprs": 0, "sgprs": 104, "sgpr_spills": 80, "vgpr_spills": 0, "scratch_bytes_per_lane": 80,
                         "lds_bytes_per_block": 58640, "occupancy_waves_per_simd": 2, "block": 256},
          "k_nl_frontier": {"vgprs": 112, "agprs": 0, "sgprs": 106, "sgpr_spills": 27, "vgpr_spills": 0, "scratch_bytes_per_lane": 0,
                            "lds_bytes_per_block": 8304, "occupancy_waves_per_simd": 4, "block": 256}}
SEED, ROLLOUTS, BIAS, PRIOR = 7, 16, 5.0, 16384.0


class Table:
    """the exported blueprint as the model reads it"""

    def __init__(self, past, present, choices, enc):
        self.rows = {(int(p), int(q), int(c)): enc[i] for i, (p, q, c) in enumerate(zip(past, present, choices))}

    def enc(self, key):
        return self.rows.get(key)

    def get(self, key):
        row = self.rows.get(key)
        return None if row is None else row["weight"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cap-log2", type=int, default=20)
    ap.add_argument("--train-steps", type=int, default=4)
    ap.add_argument("--train-batch", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--batches", default="1,64,4096")
    ap.add_argument("--iterations", default="64,8")
    ap.add_argument("--model-entries", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(R, "profiles", "nlhe_depth_rate.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import nlhe_depth_model as DM
    import oracle_nlhe as ON
    from robopoker_amd.nlhe import DEPTH_RESULT_DTYPE, Frontier, NlheSolver

    if not torch.cuda.is_available():
        raise SystemExit("nlhe_depth_rate.py measures on the GPU: no device visible")
    rng = np.random.default_rng(2026)
    to_flop = [ON.Open(2), ON.E_CALL, ON.E_DRAW]
    entries, leaves = [], []
    for _ in range(args.distinct):
        c = [int(x) for x in rng.permutation(52)[:7]]
        holes, flop = (1 << c[0] | 1 << c[1], 1 << c[2] | 1 << c[3]), 1 << c[4] | 1 << c[5] | 1 << c[6]
        entries.append(Frontier(holes, 0, [flop], to_flop))
        leaves.append(Frontier(holes, 0, [flop], to_flop + [ON.E_CHECK, ON.E_CHECK]))

    leaves_packed = Frontier.pack(leaves)
    s = NlheSolver(cap_log2=args.cap_log2, batch=args.train_batch, seed=1)
    for _ in range(args.train_steps):
        s.step("composed")
    keys, epoch = s.counters()[2], s.epoch
    say(f"table: 2^{args.cap_log2} rows, {keys} infosets after {args.train_steps} steps of {args.train_batch} trees")

    # ---- the answers against the model
    table = Table(*s.export())
    m = args.model_entries
    res, rows = s.depth_solve(entries[:m], 0, 2, ROLLOUTS, BIAS, PRIOR, SEED, 0, 32)
    t0 = time.perf_counter()
    equal = True
    for i in range(m):
        want = DM.solve(entries[i], 0, table, i, 2, bp_epoch=epoch, rollouts=ROLLOUTS, bias=BIAS,
                        prior=PRIOR, seed=SEED, first_id=0)
        for f in ("status", "past", "present", "choices", "n_actions", "iterations", "n_rows", "nodes", "infosets", "frontiers", "rollouts"):
            equal = equal and int(res[i][f]) == int(want[f])
        for f in ("refined", "regret", "sum_regret"):
            equal = equal and np.asarray(res[i][f], np.float32).tobytes() == np.asarray(want[f], np.float32).tobytes()
        equal = equal and bool(np.array_equal(res[i]["visits"], want["visits"]))
        for x, (kind, n_actions, past, present, choices, enc) in enumerate(want["rows"][:32]):
            r = rows[i][x]
            equal = equal and (int(r["kind"]), int(r["n_actions"]), int(r["past"]), int(r["present"]), int(r["choices"])) == (kind, n_actions, past, present, choices)
            equal = equal and r["enc"].tobytes() == np.asarray(enc, r["enc"].dtype).tobytes()
    model_s = time.perf_counter() - t0
    say(f"model: {m} entries x 2 iterations in {model_s:.1f} s; same bits: {equal}")

    out = {"device": torch.cuda.get_device_name(0), "cap_log2": args.cap_log2, "infosets": int(keys), "train_steps": args.train_steps,
           "train_batch": args.train_batch, "distinct_entries": args.distinct, "rollouts": ROLLOUTS, "runs": args.runs, "static_resources": STATIC,
           "model_bits_equal": bool(equal), "model_entries": m, "model_seconds": model_s,
           "timing": "host clock; solve and frontier: _device forms, from the call to rp_nlhe_sync; host_route: per iteration one "
                     "rp_nlhe_frontier_payoffs_device launch and one rp_nlhe_sync, nothing else; alternating; median / min / max of the runs",
           "results": {}}
    for n in [int(b) for b in args.batches.split(",")]:
        idx = np.arange(n) % args.distinct
        en = torch.from_numpy(NlheSolver.depth_entries([entries[i] for i in idx]).view(np.uint8).copy()).to("cuda")
        og = torch.zeros(n, dtype=torch.int8, device="cuda")
        per_batch = {}
        for iterations in [int(x) for x in args.iterations.split(",")]:
            def solve():
                t0 = time.perf_counter()
                ans = s.depth_solve_device(en, og, iterations, ROLLOUTS, BIAS, PRIOR, SEED, 0, 0)
                s.sync()
                return time.perf_counter() - t0, ans

            _, got = solve()  # warm-up, and what the solves did
            r = got[0].cpu().numpy().view(DEPTH_RESULT_DTYPE).reshape(n)
            ok = r["status"] == 0
            frontiers = int(r["frontiers"][ok].sum())
            per_tree = max(1, int(round(frontiers / max(1, int(r["iterations"][ok].sum())))))
            fr_all = torch.from_numpy(np.resize(leaves_packed, max(frontiers, 1)).view(np.uint8).reshape(-1, 112).copy()).to("cuda")
            fr_one = fr_all[:per_tree].contiguous()

            def floor():
                t0 = time.perf_counter()
                ans = s.frontier_payoffs_device(fr_all, BIAS, ROLLOUTS, SEED, 0)
                s.sync()
                return time.perf_counter() - t0, ans

            def host_route():
                t0 = time.perf_counter()
                for t in range(iterations):
                    s.frontier_payoffs_device(fr_one, BIAS, ROLLOUTS, SEED, t)
                    s.sync()
                return time.perf_counter() - t0, None

            floor()
            host_route()
            ts, tf, th = [], [], []
            for _ in range(args.runs):
                ts.append(solve()[0])
                tf.append(floor()[0])
                th.append(host_route()[0])
            statuses = {int(k): int(v) for k, v in zip(*np.unique(r["status"], return_counts=True))}
            entry = {"solves": n, "solves_ok": int(ok.sum()), "statuses": statuses, "iterations_done": int(r["iterations"][ok].sum()),
                     "frontiers": frontiers, "rollouts_played": int(r["rollouts"][ok].sum()), "nodes": int(r["nodes"][ok].sum()),
                     "max_rows": int(r["n_rows"].max()), "frontiers_per_tree": per_tree}
            for name, tt in (("solve", ts), ("frontier", tf), ("host_route_one_solve_lower_bound", th)):
                med = float(np.median(tt))
                entry[name] = {"seconds": tt, "median_s": med, "min_s": min(tt), "max_s": max(tt)}
            med = entry["solve"]["median_s"]
            entry["solve"].update(solves_per_s=n / med, iterations_per_s=entry["iterations_done"] / med, rollouts_per_s=entry["rollouts_played"] / med)
            entry["frontier"]["rollouts_per_s"] = max(frontiers, 1) * 16 * ROLLOUTS / entry["frontier"]["median_s"]
            per_batch[f"iterations_{iterations}"] = entry
            say(f"batch {n}, {iterations} iterations: solve {med * 1e3:.3f} ms [{min(ts) * 1e3:.3f}, {max(ts) * 1e3:.3f}] ({entry['solves_ok']} ok, statuses "
                f"{statuses}, {frontiers} frontiers), frontier floor {entry['frontier']['median_s'] * 1e3:.3f} ms, host route of one solve >= "
                f"{entry['host_route_one_solve_lower_bound']['median_s'] * 1e3:.3f} ms")
        out["results"][str(n)] = per_batch
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps({"model_bits_equal": out["model_bits_equal"],
                      **{f"{b}x{k}": {"solve_ms": e["solve"]["median_s"] * 1e3, "solves_ok": e["solves_ok"], "rollouts_per_s": e["solve"]["rollouts_per_s"]}
                         for b, r in out["results"].items() for k, e in r.items()}}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Rate of the safe subgame re-solve (rp_nlhe_subgame_solve, csrc/nlmc_subgame.hpp) against the depth-limited re-solve it extends: what
the per-iteration deal, the world tag and the four-world harvest cost.

Workload: scripts/nlhe_depth_rate.py's — the same 64 flop entries (open, call, the flop, seat 0 to act), the same trained table,
rollouts = 16, batches 1, 64 and 4 096, `--iterations` 64 and 8; larger batches repeat the entries, each with an id of its own.  The
beliefs come from rp_nlhe_belief_device once, before any timed window, and stay in device memory.

  subgame     rp_nlhe_subgame_solve_device at RP_NLHE_SUBGAME_ORIGIN_NONE and at origin = street - 1, one launch per 1 024 solves,
              timed from the call to rp_nlhe_sync.
  depth       rp_nlhe_depth_solve_device on the same entries (their own holes), iterations and rollouts: the entry's street against
              ORIGIN_NONE (neither has a frontier), street - 1 against street - 1.  `ratio` = subgame / depth, medians.
  depth_parent, subgame_parent  with --parent-lib: the same two solves through the PARENT commit's library, loaded beside this one, over a
              copy of the same table, in the same alternating runs at every batch — this build, the parent, this build, the parent, so
              that every timed call follows one over the other build's table.  `*_equals_parent_bytes`: the result bytes;
              `*_within_parent_spread`: this build's median inside the parent's own min - max, the noise of the host clock.
All are timed with a host clock, alternating, `--runs` runs each after a warm-up of every shape; median, min and max.
`model_bits_equal`: the first entries solved for 2 iterations against tests/nlhe_subgame_model.py over the exported table and the
device's belief — result, rows and deals.  For the whole run: mean attempts per deal, the share of fallbacks, the largest row count.

    nlhe_subgame_rate.py [--cap-log2 20] [--runs 5] [--batches 1,64,4096] [--iterations 64,8] [--parent-lib PATH]
                         [--out profiles/nlhe_subgame_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
sys.path.insert(0, os.path.join(R, "scripts"))
say = lambda m: print(m, file=sys.stderr, flush=True)  # noqa: E731

# as hipcc -Rpass-analysis=kernel-resource-usage reports them for gfx950 (csrc/Makefile's flags)
STATIC = {"k_nl_subgame": {"vgprs": 148, "agprs": 0, "sgprs": 104, "sgpr_spills": 85, "vgpr_spills": 0, "scratch_bytes_per_lane": 80,
                           "lds_bytes_per_block": 61128, "occupancy_waves_per_simd": 2, "block": 256},
          "k_nl_depth": {"vgprs": 146, "agprs": 0, "sgprs": 104, "sgpr_spills": 80, "vgpr_spills": 0, "scratch_bytes_per_lane": 80,
                         "lds_bytes_per_block": 58640, "occupancy_waves_per_simd": 2, "block": 256}}
SEED, ROLLOUTS, BIAS, PRIOR = 7, 16, 5.0, 16384.0


def parent_solver(path, like, table, epoch, cap_log2, batch):
    """an NlheSolver over ANOTHER build of the library (the parent commit's), holding a copy of `like`'s table"""
    from robopoker_amd import _lib
    from robopoker_amd.nlhe import NlheSolver

    lib = C.CDLL(path)
    for name, (res, args) in _lib._SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    own = _lib.load
    _lib.load = lambda: lib
    try:
        s = NlheSolver(cap_log2=cap_log2, batch=batch, seed=1)
    finally:
        _lib.load = own
    s.load(*table, epoch=epoch)
    return s


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
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(R, "profiles", "nlhe_subgame_rate.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import nlhe_subgame_model as SM
    from nlhe_solve_common import Table
    from nlhe_subgame_caps import flop_entries
    from robopoker_amd import _lib
    from robopoker_amd.nlhe import DEPTH_RESULT_DTYPE, SUBGAME_RESULT_DTYPE, NlheSolver

    if not torch.cuda.is_available():
        raise SystemExit("nlhe_subgame_rate.py measures on the GPU: no device visible")
    entries = flop_entries(args.distinct)
    s = NlheSolver(cap_log2=args.cap_log2, batch=args.train_batch, seed=1)
    for _ in range(args.train_steps):
        s.step("composed")
    keys, epoch = s.counters()[2], s.epoch
    say(f"table: 2^{args.cap_log2} rows, {keys} infosets after {args.train_steps} steps of {args.train_batch} trees")
    exported = s.export()
    sp = parent_solver(args.parent_lib, s, exported, epoch, args.cap_log2, args.train_batch) if args.parent_lib else None

    def to_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to("cuda")

    # ---- the answers against the model, over the device's own belief
    table = Table(*exported)
    m = args.model_entries
    bel = s.belief(NlheSolver.subgame_recalls(entries[:m]))
    res, rows, deals = s.subgame_solve(entries[:m], bel, [0, None] * (m // 2) + [0] * (m % 2), 2, ROLLOUTS, BIAS, PRIOR, SEED, 0, 48, 2)
    t0 = time.perf_counter()
    equal = not bel["status"].any()
    for i in range(m):
        want = SM.solve(entries[i], bel["hole_world"][i], bel["weights"][i], 0 if i % 2 == 0 else None, table, i, 2, bp_epoch=epoch,
                        rollouts=ROLLOUTS, bias=BIAS, prior=PRIOR, seed=SEED, first_id=0)
        for f in ("status", "past", "present", "choices", "n_actions", "iterations", "n_rows", "nodes", "infosets", "frontiers", "rollouts",
                  "attempts", "fallbacks"):
            equal = equal and int(res[i][f]) == int(want[f])
        for f in ("refined", "regret", "sum_regret"):
            equal = equal and np.asarray(res[i][f], np.float32).tobytes() == np.asarray(want[f], np.float32).tobytes()
        equal = equal and bool(np.array_equal(res[i]["visits"], want["visits"])) and list(res[i]["drawn"]) == want["drawn"]
        equal = equal and [(int(d["hole"]), int(d["world"]), int(d["attempts"])) for d in deals[i]] == want["deals"]
        for x, (world, kind, n_actions, past, present, choices, enc) in enumerate(want["rows"][:48]):
            r = rows[i][x]
            equal = equal and (int(r["world"]), int(r["kind"]), int(r["n_actions"]), int(r["past"]), int(r["present"]), int(r["choices"])) == \
                (world, kind, n_actions, past, present, choices)
            equal = equal and r["enc"].tobytes() == np.asarray(enc, r["enc"].dtype).tobytes()
    model_s = time.perf_counter() - t0
    say(f"model: {m} entries x 2 iterations in {model_s:.1f} s; same bits: {bool(equal)}")

    out = {"device": torch.cuda.get_device_name(0), "cap_log2": args.cap_log2, "infosets": int(keys), "train_steps": args.train_steps,
           "train_batch": args.train_batch, "distinct_entries": args.distinct, "rollouts": ROLLOUTS, "runs": args.runs, "static_resources": STATIC,
           "model_bits_equal": bool(equal), "model_entries": m, "model_seconds": model_s, "parent_lib": bool(sp),
           "timing": "host clock; _device forms, from the call to rp_nlhe_sync; the beliefs computed once before; alternating; median / min / "
                     "max of the runs", "results": {}}
    total_deals = total_attempts = total_fallbacks = 0
    largest_rows = 0
    batches = [int(b) for b in args.batches.split(",")]
    for n in batches:
        idx = np.arange(n) % args.distinct
        en = to_dev(NlheSolver.depth_entries([entries[i] for i in idx]))
        belief = s.belief_device(to_dev(NlheSolver.subgame_recalls([entries[i] for i in idx])))  # once, outside every window
        s.sync()
        hw, wt = belief["hole_world"], belief["weights"]
        origin = {"street_minus_1": (torch.zeros(n, dtype=torch.int8, device="cuda"), torch.zeros(n, dtype=torch.int8, device="cuda")),
                  "origin_none": (torch.full((n,), _lib.RP_NLHE_SUBGAME_ORIGIN_NONE, dtype=torch.int8, device="cuda"),
                                  torch.full((n,), _lib.RP_NLHE_DEPTH_ORIGIN_ENTRY, dtype=torch.int8, device="cuda"))}
        per_batch = {}
        for iterations in [int(x) for x in args.iterations.split(",")]:
            for name, (og_sub, og_depth) in origin.items():
                def subgame(solver=s):
                    t0 = time.perf_counter()
                    ans = solver.subgame_solve_device(en, hw, wt, og_sub, iterations, ROLLOUTS, BIAS, PRIOR, SEED, 0, 0, 0)
                    solver.sync()
                    return time.perf_counter() - t0, ans

                def depth(solver=s):
                    t0 = time.perf_counter()
                    ans = solver.depth_solve_device(en, og_depth, iterations, ROLLOUTS, BIAS, PRIOR, SEED, 0, 0)
                    solver.sync()
                    return time.perf_counter() - t0, ans

                with_parent = sp is not None
                _, got = subgame()  # warm-up, and what the solves did
                _, got_depth = depth()
                if with_parent:
                    _, got_parent = depth(sp)
                    same_as_parent = got_parent[0].cpu().numpy().tobytes() == got_depth[0].cpu().numpy().tobytes()
                    subgame_same_as_parent = subgame(sp)[1][0].cpu().numpy().tobytes() == got[0].cpu().numpy().tobytes()
                r = got[0].cpu().numpy().view(SUBGAME_RESULT_DTYPE).reshape(n)
                rd = got_depth[0].cpu().numpy().view(DEPTH_RESULT_DTYPE).reshape(n)
                ok = r["status"] == 0
                ts, td, tp, tsp = [], [], [], []
                for _ in range(args.runs):
                    # the two builds hold a table each, and a call that follows one over its own table finds it cached: with the parent,
                    # every timed call of either build follows one over the OTHER build's table
                    ts.append(subgame()[0])
                    if with_parent:
                        tsp.append(subgame(sp)[0])
                    td.append(depth()[0])
                    if with_parent:
                        tp.append(depth(sp)[0])
                statuses = {int(k): int(v) for k, v in zip(*np.unique(r["status"], return_counts=True))}
                done = int(r["iterations"][ok].sum())
                total_deals += done
                total_attempts += int(r["attempts"][ok].sum())
                total_fallbacks += int(r["fallbacks"][ok].sum())
                largest_rows = max(largest_rows, int(r["n_rows"].max()))
                entry = {"solves": n, "solves_ok": int(ok.sum()), "statuses": statuses, "iterations_done": done,
                         "frontiers": int(r["frontiers"][ok].sum()), "rollouts_played": int(r["rollouts"][ok].sum()), "nodes": int(r["nodes"][ok].sum()),
                         "max_rows": int(r["n_rows"].max()), "depth_max_rows": int(rd["n_rows"].max()), "depth_statuses":
                         {int(k): int(v) for k, v in zip(*np.unique(rd["status"], return_counts=True))},
                         "attempts_per_deal": float(r["attempts"][ok].sum()) / max(done, 1), "fallbacks": int(r["fallbacks"][ok].sum()),
                         "drawn": [int(x) for x in r["drawn"][ok].sum(axis=0)]}
                for key, tt in (("subgame", ts), ("depth", td)) + ((("depth_parent", tp), ("subgame_parent", tsp)) if with_parent else ()):
                    entry[key] = {"seconds": tt, "median_s": float(np.median(tt)), "min_s": min(tt), "max_s": max(tt)}
                entry["ratio"] = entry["subgame"]["median_s"] / entry["depth"]["median_s"]
                entry["subgame"]["iterations_per_s"] = done / entry["subgame"]["median_s"]
                if with_parent:
                    entry["depth_equals_parent_bytes"] = bool(same_as_parent)
                    entry["depth_over_parent"] = entry["depth"]["median_s"] / entry["depth_parent"]["median_s"]
                    entry["subgame_equals_parent_bytes"] = bool(subgame_same_as_parent)
                    entry["subgame_over_parent"] = entry["subgame"]["median_s"] / entry["subgame_parent"]["median_s"]
                    for kind in ("depth", "subgame"):  # this build's median inside the parent's own spread of the same alternating runs
                        own, par = entry[kind], entry[kind + "_parent"]
                        entry[kind + "_within_parent_spread"] = bool(par["min_s"] <= own["median_s"] <= par["max_s"])
                        entry[kind + "_above_parent_max"] = bool(own["median_s"] > par["max_s"])
                per_batch[f"iterations_{iterations}_{name}"] = entry
                say(f"batch {n}, {iterations} iterations, {name}: subgame {entry['subgame']['median_s'] * 1e3:.3f} ms [{min(ts) * 1e3:.3f}, "
                    f"{max(ts) * 1e3:.3f}], depth {entry['depth']['median_s'] * 1e3:.3f} ms [{min(td) * 1e3:.3f}, {max(td) * 1e3:.3f}], ratio "
                    f"{entry['ratio']:.2f}; {entry['solves_ok']} ok, statuses {statuses}, max rows {entry['max_rows']} (depth {entry['depth_max_rows']}), "
                    f"{entry['attempts_per_deal']:.2f} attempts per deal, {entry['fallbacks']} fallbacks"
                    + (f"; parent's depth {entry['depth_parent']['median_s'] * 1e3:.3f} ms [{min(tp) * 1e3:.3f}, {max(tp) * 1e3:.3f}], same bytes "
                       f"{same_as_parent}; parent's subgame {entry['subgame_parent']['median_s'] * 1e3:.3f} ms [{min(tsp) * 1e3:.3f}, "
                       f"{max(tsp) * 1e3:.3f}], same bytes {subgame_same_as_parent}" if with_parent else ""))
        out["results"][str(n)] = per_batch
    out["whole_run"] = {"deals": total_deals, "mean_attempts_per_deal": total_attempts / max(total_deals, 1),
                        "fallback_share": total_fallbacks / max(total_deals, 1), "largest_row_count": largest_rows,
                        "row_cap": _lib.RP_NLHE_SUBGAME_MAX_ROWS}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps({"model_bits_equal": out["model_bits_equal"], "whole_run": out["whole_run"],
                      **{f"{b}x{k}": {"subgame_ms": e["subgame"]["median_s"] * 1e3, "depth_ms": e["depth"]["median_s"] * 1e3, "ratio": e["ratio"],
                                      "solves_ok": e["solves_ok"]} for b, r in out["results"].items() for k, e in r.items()}}))


if __name__ == "__main__":
    main()

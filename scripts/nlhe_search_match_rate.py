#!/usr/bin/env python3
"""Rate of search matches on the device (rp_nlhe_search_match, csrc/nlmc_search.hpp), and what the rounds cost.

Workload: heads-up hands from the deal to the settlement, stacks 200, alternating dealer, World<Blueprint> on seat 0 against the plain
blueprint agent on seat 1, both reading one table.  The blueprint is the library's own: `--train-steps` steps of the NLHE solver on
128 trees fill the table with real infosets before anything is timed.

  search    rp_nlhe_search_match_device at `--hands` hands and `--iterations` iterations per solve, the reference's defaults otherwise
            (16 rollouts, bias 5, prior 2^14, visit_threshold 2^18, origin none): hands/s, solves/s, rounds' share.
  bare      rp_nlhe_belief_device + rp_nlhe_subgame_solve_device + sync on the recalls the match traced (every solve of the match,
            one batch, ids first_id + i): the time the two kernels need for the same requests without rounds.  search - bare is the cost
            of the rounds, the compaction, the per-round synchronisation and the small launches of late rounds.
  match     rp_nlhe_match (host form) at the same number of hands, in child processes that load `--parent-lib` (the parent commit's
            build) and this tree's library alternately: the shared loop body must cost the match kernel nothing.  At that size the call
            is launches and copies, so each child also times rp_nlhe_match_device + sync at `--large-hands` hands, where the kernel shows.
Timed with a host clock around calls that end in a device synchronise, `--runs` runs each after a warm-up; median, min and max.

    nlhe_search_match_rate.py [--hands 4096] [--iterations 64] [--runs 5] [--train-steps 2000] [--parent-lib PATH] [--out profiles/nlhe_search_match_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
say = lambda m: print(m, file=sys.stderr, flush=True)  # noqa: E731
SEED = 2026


def timed(fn, runs):
    fn()  # warm-up
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def figures(ts):
    import numpy as np

    return {"seconds": ts, "median_s": float(np.median(ts)), "min_s": min(ts), "max_s": max(ts)}


def trained(args):
    from robopoker_amd.nlhe import NlheSolver

    s = NlheSolver(cap_log2=args.cap_log2, batch=128, seed=1)
    for _ in range(args.train_steps):
        s.step()
    s.sync()
    return s


def match_only(args):
    """a child process: rp_nlhe_match of the library at --lib, one JSON line"""
    import torch

    from robopoker_amd import _lib

    if args.lib:
        lib = C.CDLL(args.lib)
        for name, (res, a) in _lib._SIGNATURES.items():
            if hasattr(lib, name):  # the parent's build has no search match
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, a
        _lib._lib = lib
    s = trained(args)
    got = s.match(args.hands, seed=SEED)
    ts = timed(lambda: s.match(args.hands, seed=SEED), args.runs)

    # at --hands the call is launches and copies; the kernel itself shows at a batch that fills the device, outputs kept there
    def large():
        out = s.match_device(args.large_hands, seed=SEED)
        s.sync()
        return out

    big = large()
    big_ts = timed(large, args.runs)
    print(json.dumps(dict(figures(ts), won_sum=int(got["won"].astype("int64").sum()), plays=int(got["hands"]["n_plays"].sum()), keys=int(s.counters()[2]),
                          large=dict(figures(big_ts), hands=args.large_hands, won_sum=int(big["won"].sum(dtype=torch.int64).item())))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hands", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--train-steps", type=int, default=2000)
    ap.add_argument("--cap-log2", type=int, default=20)
    ap.add_argument("--steps-cap", type=int, default=48, help="traced decisions per hand; at RP_NLHE_SEARCH_MAX_SOLVES every solve is traced")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the two libraries")
    ap.add_argument("--large-hands", type=int, default=1 << 20, help="the batch of the device-form comparison of the two libraries")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--match-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "nlhe_search_match_rate.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("nlhe_search_match_rate.py measures on the GPU: no device visible")
    if args.match_only:
        return match_only(args)

    from robopoker_amd.nlhe import FRONTIER_DTYPE, RECALL_DTYPE, SEARCH_STEP_DTYPE

    s = trained(args)
    n = args.hands
    kw = dict(seed=SEED, search=("world", "none"), iterations=args.iterations, search_seed=SEED + 1)
    say(f"table: 2^{args.cap_log2} slots, {s.counters()[2]} infosets after {args.train_steps} steps")

    traced = s.search_match_device(n, steps_cap=args.steps_cap, **kw)
    steps = traced["steps"].cpu().numpy().reshape(-1).view(SEARCH_STEP_DTYPE).reshape(n, -1)
    searched, unsolved = traced["searched"].cpu().numpy().astype(np.int64), traced["unsolved"].cpu().numpy().astype(np.int64)
    asked = steps[(steps["recall"]["hole"] != 0)]  # a step that asked for a solve holds its recall; fallbacks LENGTH and CAP hold none
    solves = int(asked.size)
    # a hand past the trace may have asked for solves that are not counted: none can be with --steps-cap 48, the cap of solves per hand
    untraced = int((searched > args.steps_cap).sum())
    # a chunk of 1 024 hands plays one round per solve of its longest hand, and one more in which the last hands end
    per_hand = (steps["recall"]["hole"] != 0).sum(axis=1)
    rounds = [int(per_hand[at:at + 1024].max()) + 1 for at in range(0, n, 1024)]
    say(f"{n} hands: {int(searched.sum())} search decisions, {solves} solves traced, {int(unsolved.sum())} fell back; "
        f"fallback codes {np.bincount(steps['fallback'][steps['solve_id'] != 0], minlength=6).tolist()}")
    search = figures(timed(lambda: s.search_match_device(n, **kw), args.runs))
    plain = figures(timed(lambda: s.match(n, seed=SEED), args.runs))

    # ---- the bare calls on the traced requests
    rec = np.ascontiguousarray(asked["recall"])
    ent = np.zeros(solves, FRONTIER_DTYPE)
    for f in ("draws", "stacks", "dealer", "n_edges", "edges"):
        ent[f] = rec[f]
    ent["internal"] = rec["pov"]
    ent["holes"][np.arange(solves), rec["pov"]] = rec["hole"]
    for i in range(solves):
        e = [int(x) for x in rec["edges"][i, : rec["n_edges"][i]]]
        tail = (e[len(e) - e[::-1].index(1):] if 1 in e else e)[:12]
        ent["n_prefix"][i], ent["prefix"][i, : len(tail)] = len(tail), tail
    rec_dev = torch.from_numpy(rec.view(np.uint8).reshape(solves, RECALL_DTYPE.itemsize)).to("cuda")
    ent_dev = torch.from_numpy(ent.view(np.uint8).reshape(solves, FRONTIER_DTYPE.itemsize)).to("cuda")

    def bare():
        b = s.belief_device(rec_dev)
        out = s.subgame_solve_device(ent_dev, b["hole_world"], b["weights"], None, args.iterations, seed=SEED + 1)
        s.sync()
        return out

    bare_t = figures(timed(bare, args.runs))

    def belief_alone():
        s.belief_device(rec_dev)
        s.sync()

    belief_t = figures(timed(belief_alone, args.runs))
    out = {"device": torch.cuda.get_device_name(0), "hands": n, "iterations": args.iterations, "runs": args.runs, "train_steps": args.train_steps,
           "infosets": int(s.counters()[2]),
           "timing": "host clock around calls that end in a device synchronise; a warm-up, then the runs; median / min / max",
           "search_decisions": int(searched.sum()), "solves": solves, "fell_back": int(unsolved.sum()),
           "fallback_codes": np.bincount(steps["fallback"][steps["solve_id"] != 0], minlength=6).tolist(),
           "solve_status_counts": np.bincount(asked["result"]["status"], minlength=12).tolist(),
           "steps_cap": args.steps_cap, "hands_with_decisions_past_the_trace": untraced,
           "rounds_per_chunk_of_1024": rounds, "synchronisations": sum(rounds),
           "search_match": dict(search, hands_per_s=n / search["median_s"], solves_per_s=solves / search["median_s"]),
           "plain_match_same_hands": dict(plain, hands_per_s=n / plain["median_s"]),
           "bare_belief_plus_subgame": dict(bare_t, solves_per_s=solves / bare_t["median_s"]),
           "bare_belief_alone": belief_t,
           "share_of_wall_time_in_the_two_kernels": bare_t["median_s"] / search["median_s"],
           "cost_of_the_rounds_s": search["median_s"] - bare_t["median_s"]}
    say(f"search match {search['median_s'] * 1e3:.1f} ms [{search['min_s'] * 1e3:.1f}, {search['max_s'] * 1e3:.1f}] = {n / search['median_s']:.4g} hands/s, "
        f"{solves / search['median_s']:.4g} solves/s; bare {bare_t['median_s'] * 1e3:.1f} ms (belief {belief_t['median_s'] * 1e3:.1f}); "
        f"plain match {plain['median_s'] * 1e3:.3f} ms")

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)  # kept if the comparison below is cut short

    # ---- rp_nlhe_match, the parent's build and this one alternately, each in a process of its own
    if args.parent_lib:
        runs = {"parent": [], "this": []}
        for r in range(args.rounds):
            for name, lib in (("parent", args.parent_lib), ("this", None)):
                cmd = [sys.executable, os.path.abspath(__file__), "--match-only", "--hands", str(n), "--runs", str(args.runs), "--train-steps",
                       str(args.train_steps), "--cap-log2", str(args.cap_log2), "--large-hands", str(args.large_hands)] + (["--lib", lib] if lib else [])
                line = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout.strip().splitlines()[-1]
                runs[name].append(json.loads(line))
                say(f"match {name} round {r}: {runs[name][-1]['median_s'] * 1e3:.3f} ms; {args.large_hands} hands on the device "
                    f"{runs[name][-1]['large']['median_s'] * 1e3:.3f} ms")
        out["match_before_after"] = {k: {"per_process": v, "median_of_medians_s": float(np.median([x["median_s"] for x in v])),
                                         "min_s": min(x["min_s"] for x in v), "max_s": max(x["max_s"] for x in v)} for k, v in runs.items()}
        out["match_before_after_device_form"] = {
            k: {"hands": args.large_hands, "median_of_medians_s": float(np.median([x["large"]["median_s"] for x in v])),
                "min_s": min(x["large"]["min_s"] for x in v), "max_s": max(x["large"]["max_s"] for x in v)} for k, v in runs.items()}
        out["match_before_after_device_form"]["same_answers"] = len({x["large"]["won_sum"] for v in runs.values() for x in v}) == 1
        out["match_before_after"]["same_answers"] = len({(x["won_sum"], x["plays"], x["keys"]) for v in runs.values() for x in v}) == 1
        json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps({k: out[k] for k in ("search_match", "share_of_wall_time_in_the_two_kernels")}))


if __name__ == "__main__":
    main()

"""Solve-iterations per second of the table-game re-solves on Leduc (root entries over the 30 deals in turn, W = 2, 4 096 iterations, n =
64, 1 024, 8 192 solves), three variants alternating in one run, five repeats each, by the library's kernel clock (rp_mccfr_profile /
rp_mccfr_kernel_time "subgame"):

    subgame        rp_mccfr_subgame_solve                      the kernel's FR = false instantiation
    depth_none     rp_mccfr_depth_solve, origin NONE           the FR = true instantiation growing no frontier: the same answer
    depth_origin0  rp_mccfr_depth_solve, origin 0, D = 4       the board deal is a frontier: the 4 x 4 continuation game below it

with the nodes per iteration of each.  Writes profiles/mccfr_depth_rate.json and prints the DESIGN table.  Recorded, not gated.

    python scripts/mccfr_depth_rate.py [out.json]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (first: one HIP runtime per process)

from robopoker_amd import Game, _lib, games  # noqa: E402
from robopoker_amd.mccfr import Solver  # noqa: E402

ITERATIONS, WORLDS, SIZES, REPEATS, LEAVES = 4096, 2, (64, 1024, 8192), 5, 4
DEALS = [(a, b) for a in range(6) for b in range(6) if a != b]


def main():
    game = Game("leduc")
    solver = Solver(game, "floored", "linear", "external", batch=1, seed=0).solve(1 << 12)
    f = games.frontiers(game)
    solver.set_frontiers(f["depth"], f["pick_info"], f["payoff_ref"], leaves=LEAVES)
    priors, entries = zip(*(games.subgame_entry(game, holes, (), 1, n_worlds=WORLDS) for holes in DEALS))
    entries = games.fill_belief(np.concatenate(entries), solver.subgame_belief(np.concatenate(priors)))
    variants = {"subgame": lambda batch: solver.subgame_solve(batch, iterations=ITERATIONS, seed=1),
                "depth_none": lambda batch: solver.depth_solve(batch, _lib.RP_MCCFR_ORIGIN_NONE, iterations=ITERATIONS, seed=1),
                "depth_origin0": lambda batch: solver.depth_solve(batch, 0, iterations=ITERATIONS, seed=1)}
    for run in variants.values():  # first launches: code objects
        run(entries[:1])
    solver.profile(True)
    out = {"game": "leduc", "entry": "root, external 1", "iterations": ITERATIONS, "n_worlds": WORLDS, "leaves": LEAVES, "repeats": REPEATS,
           "unit": "solve-iterations per second, kernel clock", "solves": {}}
    for n in SIZES:
        batch = entries[np.arange(n) % len(entries)]
        times = {name: [] for name in variants}
        nodes, answers = {}, {}
        for _ in range(REPEATS):
            for name, run in variants.items():  # alternating, so that drift lands on all three
                before = solver.kernel_time("subgame")[0]
                results, _ = run(batch)
                times[name].append((solver.kernel_time("subgame")[0] - before) / 1e3)
                assert not results["status"].any()
                nodes[name] = float(results["nodes"].mean()) / ITERATIONS
                answers[name] = results.tobytes()
        assert answers["subgame"] == answers["depth_none"], "origin NONE does not answer rp_mccfr_subgame_solve's bytes"
        out["solves"][str(n)] = {
            name: {"kernel_s": [round(t, 6) for t in ts], "kernel_s_median": round(float(np.median(ts)), 6),
                   "spread": round((max(ts) - min(ts)) / float(np.median(ts)), 4),
                   "iterations_per_s": round(n * ITERATIONS / float(np.median(ts)), 1), "nodes_per_iteration": round(nodes[name], 3)}
            for name, ts in times.items()}
    solver.close()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mccfr_depth_rate.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("| solves | variant | kernel s (median of 5) | spread | solve-iterations / s | nodes / iteration |")
    print("|---|---|---|---|---|---|")
    for n, by in out["solves"].items():
        for name, r in by.items():
            print(f"| {n} | {name} | {r['kernel_s_median']:.4f} | {100 * r['spread']:.1f} % | {r['iterations_per_s']:.3g} | {r['nodes_per_iteration']:.2f} |")


if __name__ == "__main__":
    main()

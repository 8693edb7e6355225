"""Solve-iterations per second of rp_mccfr_subgame_solve (Kuhn and Leduc, W = 2, 4 096 iterations, n = 1, 64, 1 024, 8 192 solves of the
root entry over the 30 deals in turn), by the library's kernel clock (rp_mccfr_profile / rp_mccfr_kernel_time "subgame"), and for scale
the per-step time of rp_mccfr_step at batch 1 in ORDERED mode on the same handle: the closest existing thing to one subgame iteration,
which pays its launches per step.  Writes profiles/mccfr_subgame_rate.json.  Recorded, not gated.

    python scripts/mccfr_subgame_rate.py [out.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (first: one HIP runtime per process)

from robopoker_amd import Game, games  # noqa: E402
from robopoker_amd.mccfr import Solver  # noqa: E402

ITERATIONS, WORLDS, SIZES, STEPS, CLOCKED_STEPS = 4096, 2, (1, 64, 1024, 8192), 20000, 2000
DEALS = [(a, b) for a in range(6) for b in range(6) if a != b]


def main():
    out = {"iterations": ITERATIONS, "n_worlds": WORLDS, "unit": "solve-iterations per second, kernel clock"}
    for name in ("kuhn", "leduc"):
        game = Game(name)
        solver = Solver(game, "floored", "linear", "external", batch=1, seed=0)
        solver.step()  # first launches: code objects, buffers
        solver.sync()
        t0 = time.perf_counter()  # the wall time of a step without the clocks' events on the stream
        for _ in range(STEPS):
            solver.step()
        solver.sync()
        step_wall = (time.perf_counter() - t0) / STEPS
        solver.profile(True)
        for _ in range(CLOCKED_STEPS):
            solver.step()
        solver.sync()
        step_kernels = sum(solver.kernel_time(k)[0] for k in ("traverse", "compact", "update")) / 1e3 / CLOCKED_STEPS
        priors, entries = zip(*(games.subgame_entry(game, holes, (), 1, n_worlds=WORLDS) for holes in DEALS))
        entries = games.fill_belief(np.concatenate(entries), solver.subgame_belief(np.concatenate(priors)))
        solver.subgame_solve(entries[:1], iterations=8)  # first launch
        rows = {}
        for n in SIZES:
            batch = entries[np.arange(n) % len(entries)]
            before = solver.kernel_time("subgame")[0]
            t0 = time.perf_counter()
            results, _ = solver.subgame_solve(batch, iterations=ITERATIONS, seed=1)
            wall = time.perf_counter() - t0
            kernel_s = (solver.kernel_time("subgame")[0] - before) / 1e3
            assert not results["status"].any()
            rows[str(n)] = {"kernel_s": round(kernel_s, 6), "wall_s": round(wall, 6), "iterations_per_s": round(n * ITERATIONS / kernel_s, 1),
                            "s_per_iteration_of_one_solve": kernel_s / ITERATIONS, "nodes_per_iteration": float(results["nodes"].mean()) / ITERATIONS}
        out[name] = {"solves": rows,
                     "mccfr_step_batch1_ordered": {"wall_s_per_step": step_wall, "kernel_s_per_step": step_kernels, "steps": STEPS, "clocked_steps": CLOCKED_STEPS},
                     "single_solve_kernel_s_per_iteration_below_step_wall_s": rows["1"]["s_per_iteration_of_one_solve"] < step_wall,
                     "single_solve_kernel_s_per_iteration_below_step_kernel_s": rows["1"]["s_per_iteration_of_one_solve"] < step_kernels,
                     "rate_8192_over_rate_1": round(rows["8192"]["iterations_per_s"] / rows["1"]["iterations_per_s"], 1)}
        solver.close()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mccfr_subgame_rate.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

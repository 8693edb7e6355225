#!/usr/bin/env python3
"""Wall times of the best response on the device (rp_mccfr_exploitability_device, csrc/mccfr_nash.hpp) beside the host path it
restates (rp_mccfr_exploitability: the four table columns to the host, the tree expanded and walked on one core — the yardstick), on
Leduc and wide Leduc, in both launch shapes; and of rp_mccfr_solve_to beside the same loop done with rp_mccfr_solve and the host check.

Every call is timed by a host clock between two synchronisations of the solver's stream; a warm-up (code objects, and the handle's
first call builds and uploads its tree), then RUNS runs: median, minimum and maximum.  The table is the one 20 composed steps leave.

usage: mccfr_nash_rate.py [max_steps]    -> profiles/mccfr_nash_times.json and the same JSON object on stdout"""
import json
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from robopoker_amd.games import Game  # noqa: E402
from robopoker_amd.mccfr import Solver  # noqa: E402

RUNS = 5
say = lambda m: print(m, file=sys.stderr, flush=True)  # noqa: E731


def timed(s, fn):
    s.sync()
    t0 = time.perf_counter()
    out = fn()
    s.sync()
    return time.perf_counter() - t0, out


def entry(times):
    times = sorted(times)
    return {"s": round(times[len(times) // 2], 7), "min_s": round(times[0], 7), "max_s": round(times[-1], 7), "runs": len(times)}


def repeat(s, fn):
    timed(s, fn)
    return entry([timed(s, fn)[0] for _ in range(RUNS)])


def handle(game, forced):
    """a solver after 20 composed steps whose first best-response call will build the tree under RP_NASH_VARIANT = forced"""
    if forced:
        os.environ["RP_NASH_VARIANT"] = forced
    else:
        os.environ.pop("RP_NASH_VARIANT", None)
    s = Solver(game, "linear", "linear", "external", batch=1024, seed=1, mode="composed")
    s.step_async(20)
    s.sync()
    return s


out = {}
buf = torch.zeros(1, dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
for name in ("leduc", "leduc_wide"):
    game = Game(name)
    s = handle(game, None)
    natural = s.nash_variant()
    g = {"natural_variant": natural, "host": repeat(s, s.exploitability)}
    want = np.float32(s.exploitability())
    for forced in ("one", "levels"):
        d = s if forced == natural else handle(game, forced)
        g["device_" + forced] = repeat(d, lambda: d.exploitability_device(buf.data_ptr()))
        assert d.nash_variant() == forced
        assert buf.cpu().numpy().view(np.uint32)[0] == want.view(np.uint32), (name, forced)  # the same table, the same bits
    g["host_over_natural_device"] = round(g["host"]["s"] / g["device_" + natural]["s"], 1)
    g["natural_device_not_above_host"] = g["device_" + natural]["s"] <= g["host"]["s"]
    out[name] = g
    say(f"{name}: {json.dumps(g)}")
os.environ.pop("RP_NASH_VARIANT", None)

# solve to a target on Leduc, composed update: one call against the loop a caller writes today
TARGET, EVERY, BATCH, MAX_STEPS = 0.01, 8, 1024, int(sys.argv[1]) if len(sys.argv) > 1 else 40000
game = Game("leduc")


def fresh():
    return Solver(game, "linear", "linear", "external", batch=BATCH, seed=1, mode="composed")


def host_loop(s):
    steps = 0
    while steps < MAX_STEPS:
        s.solve(EVERY * BATCH)
        steps += EVERY
        if s.exploitability() < TARGET:
            break
    return steps


dev_t, host_t, result = [], [], None
for run in range(RUNS + 1):
    a, b = fresh(), fresh()
    a.nash_variant()  # the tree is static data: built outside the clock, as a long-lived handle has it
    t, got = timed(a, lambda: a.solve_to(TARGET, EVERY, MAX_STEPS))
    th, steps = timed(b, lambda: host_loop(b))
    assert got[0] == steps and np.float32(got[1]).view(np.uint32) == np.float32(b.exploitability()).view(np.uint32)
    if run:
        dev_t.append(t)
        host_t.append(th)
    result = got
    a.close()
    b.close()
out["solve_to_leduc_composed"] = {"target": TARGET, "check_every": EVERY, "batch": BATCH, "steps": result[0], "exploitability": result[1],
                                  "reached": result[2], "solve_to": entry(dev_t), "solve_plus_host_check": entry(host_t)}
out["solve_to_leduc_composed"]["host_loop_over_solve_to"] = round(entry(host_t)["s"] / entry(dev_t)["s"], 2)
os.makedirs(os.path.join(R, "profiles"), exist_ok=True)
with open(os.path.join(R, "profiles", "mccfr_nash_times.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out), flush=True)

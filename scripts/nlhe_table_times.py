#!/usr/bin/env python3
"""Wall times of moving the NLHE infoset table on the device (rp_nlhe_resize / _export_device / _import_device, csrc/nlmc_table.hpp)
beside the blueprint census' scan of the same table (the yardstick: a read-only pass over slots and rows) and beside the path that
existed before them: export() into host arrays, a new handle of twice the size, load().

A table of 2^24 slots, half full of synthetic distinct keys.  Every call is timed by a host clock between two synchronisations of the
solver's stream, allocations included (a resize allocates its new table, an export its output tensors); a warm-up, then RUNS runs:
median, minimum and maximum.  "bytes" is what the call necessarily moves: S slots of 32 B, K ready rows of 144 B, keys of 20 B and
Encounters of 144 B per infoset.

usage: nlhe_table_times.py [cap_log2]    -> profiles/nlhe_table_times.json and the same JSON object on stdout"""
import json
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from robopoker_amd.nlhe import ENC_DTYPE, NlheSolver  # noqa: E402

cap = int(sys.argv[1]) if len(sys.argv) > 1 else 24
S, K = 1 << cap, 1 << (cap - 1)
say = lambda m: print(m, file=sys.stderr, flush=True)  # noqa: E731


def timed(s, fn):
    s.sync()
    t0 = time.perf_counter()
    out = fn()
    s.sync()
    return time.perf_counter() - t0, out


RUNS = 5


def entry(times, nbytes):
    times = sorted(times)
    med = times[len(times) // 2]
    return {"s": round(med, 6), "min_s": round(times[0], 6), "max_s": round(times[-1], 6), "runs": len(times), "bytes": int(nbytes),
            "GB_per_s": round(nbytes / med / 1e9, 2)}


def repeat(s, fn, runs=RUNS):
    timed(s, fn)  # warm-up: code objects, the allocator, the handle's scratch
    return [timed(s, fn)[0] for _ in range(runs)]


# K distinct keys: a distinct `past` each; present = a flop bucket; choices = four edges (raise, shove, call, fold)
i = torch.arange(K, dtype=torch.int64, device="cuda")
past = i * (0x9E3779B97F4A7C15 - (1 << 64)) + 1  # an odd multiplier modulo 2^64 (as torch's signed 64 bits): a bijection
present = (0x0100 | (i & 0xFF)).to(torch.int32)
choices = torch.full((K,), 6 | (5 << 5) | (4 << 10) | (2 << 15), dtype=torch.int64, device="cuda")
enc = torch.rand((K, 9, 4), dtype=torch.float32, device="cuda")
enc.view(torch.int32)[:, :, 3] = (i % 1000).to(torch.int32)[:, None]  # visits
enc = enc.view(torch.uint8).reshape(K, 9, ENC_DTYPE.itemsize)
torch.cuda.synchronize()

out = {"slots": S, "infosets": K, "fill": K / S}
# load_device into an EMPTY table (every key inserted): a fresh handle per run, made outside the timed call
load_bytes = K * (164 + 32 + 32 + 144 + 8)  # keys and Encounters in, a slot read and written, the row written, the row index out and in
times = []
for run in range(RUNS + 1):
    a = NlheSolver(cap_log2=cap, batch=16, seed=1)
    times.append(timed(a, lambda: a.load_device(past, present, choices, enc, 5))[0])
    if run < RUNS:
        a.close()
out["load_device"] = entry(times[1:], load_bytes)
assert a.capacity() == (cap, K)
# ... and into the table that holds every key already (found, rows overwritten)
out["load_device_again"] = entry(repeat(a, lambda: a.load_device(past, present, choices, enc, 5)), load_bytes - K * 32)
out["census_scan"] = entry(repeat(a, a.table_census_device), S * 32 + K * 144)
out["export_device"] = entry(repeat(a, a.export_device), S * 32 + S * 32 + K * 144 + K * 164)  # the count pass, the compaction pass, rows in, keys and Encounters out
assert a.export_device(cap=1)[4] == K
up, down = [], []
for run in range(RUNS + 1):
    up.append(timed(a, lambda: a.resize(cap + 1))[0])
    assert a.capacity() == (cap + 1, K)
    down.append(timed(a, lambda: a.resize(cap))[0])
    assert a.capacity() == (cap, K)
out["resize_up"] = entry(up[1:], S * 32 + K * 144 + 2 * S * 176 + K * 176)  # old slots and rows in, the new table cleared, keys and rows written
out["resize_down"] = entry(down[1:], 2 * S * 32 + K * 144 + S * 176 + K * 176)
# the path that exists without them (unchanged code): the whole slot array to the host and a host scan, a new handle, host probing,
# the slot array down and up again, rows packed on the host
say(f"device side: {json.dumps(out)}")
t0 = time.perf_counter()
host = a.export()
t_export = time.perf_counter() - t0
t0 = time.perf_counter()
b = NlheSolver(cap_log2=cap + 1, batch=16, seed=1)
b.sync()
t_create = time.perf_counter() - t0
t0 = time.perf_counter()
b.load(*host, epoch=a.epoch)
b.sync()
t_load = time.perf_counter() - t0
assert b.capacity() == (cap + 1, K)
out["host_path"] = {"export_s": round(t_export, 4), "create_s": round(t_create, 4), "load_s": round(t_load, 4),
                    "total_s": round(t_export + t_create + t_load, 4)}
out["host_path_over_resize_up"] = round((t_export + t_create + t_load) / out["resize_up"]["s"], 1)
# the two tables hold the same blueprint
probe = np.random.default_rng(0).choice(K, min(K, 4096), replace=False)
ka = a.memory(host[0][probe], host[1][probe], host[2][probe])
kb = b.memory(host[0][probe], host[1][probe], host[2][probe])
out["same_answers_by_key"] = bool(ka[2].all() and kb[2].all() and ka[0].tobytes() == kb[0].tobytes())
a.close()
b.close()
os.makedirs(os.path.join(R, "profiles"), exist_ok=True)
with open(os.path.join(R, "profiles", "nlhe_table_times.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out), flush=True)

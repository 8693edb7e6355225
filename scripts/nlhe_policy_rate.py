#!/usr/bin/env python3
"""Rate of the blueprint queries by NlheInfo key (rp_nlhe_policy_device / rp_nlhe_memory_device) on a table of a user's size.

Setup: a table of 2^cap_log2 rows, half filled with synthetic keys through load(); 2^22 queries, a tenth of them absent keys; the
device-pointer forms on a torch stream, warmed up, then timed with device events over `launches` launches per window, the two
kernel shapes of the policy query (csrc/nlmc_query.hpp: a group of 8 lanes per query, one lane per query) alternating in `rounds`
rounds.  The answers of both shapes are compared bit for bit at the timed size, and a sample against the numpy model of
tests/nlhe_policy_model.py.  Also timed: the only route that existed before for the same answers — rp_nlhe_export of the table
plus the numpy model on the host.

    nlhe_policy_rate.py [--cap-log2 24] [--queries 4194304] [--launches 20] [--rounds 3] [--out profiles/nlhe_policy_rate.json]
    nlhe_policy_rate.py --profile-run         the timed launches alone, few of them: the program of a rocprofv3 --kernel-trace --stats run
    nlhe_policy_rate.py --merge-kernel-stats STATS.csv --out FILE.json      adds the kernel times of that run to FILE.json (no GPU)
"""
import argparse
import csv
import json
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))

HBM_PEAK = 8.0e12  # bytes/s, the MI355X's HBM3E specification
KEY_BYTES, SLOT_BYTES = 20, 32
ROW_BYTES = {"iterated": 36, "averaged": 72, "sampling": 72, "memory": 144}  # the part of the 144-byte row the answer depends on
OUT_BYTES = {"iterated": 47, "averaged": 47, "sampling": 47, "memory": 146}  # policy 36 + edges 9 + n_actions 1 + found 1; enc 144 + 2
say = lambda m: print(m, file=sys.stderr, flush=True)  # noqa: E731


def merge_kernel_stats(stats_csv, out_path):
    keep = {}
    for r in csv.DictReader(open(stats_csv)):
        name = r.get("Name", "")
        if "k_nl_policy" in name or "k_nl_memory" in name:
            calls, total = int(r["Calls"]), float(r["TotalDurationNs"])
            keep[name.split("(")[0]] = {"calls": calls, "average_us": total / calls / 1e3, "min_us": float(r["MinNs"]) / 1e3, "max_us": float(r["MaxNs"]) / 1e3}
    out = json.load(open(out_path))
    out["kernel_time_rocprofv3"] = {"source": "rocprofv3 --kernel-trace --stats, a run of its own (--profile-run)", "kernels": keep}
    json.dump(out, open(out_path, "w"), indent=1)
    print(json.dumps(out["kernel_time_rocprofv3"]))


def synthetic_table(rng, n):
    import numpy as np

    from robopoker_amd.nlhe import A, ENC_DTYPE

    past = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    present = rng.integers(0, 1 << 16, n, dtype=np.uint32)
    nch = rng.integers(1, A + 1, n)
    choices = np.zeros(n, np.uint64)
    for a in range(A):
        choices |= np.where(a < nch, rng.integers(2, 16, n).astype(np.uint64) << np.uint64(5 * a), np.uint64(0))
    enc = np.zeros((n, A), dtype=ENC_DTYPE)
    enc["regret"] = rng.standard_normal((n, A), dtype=np.float32) * 100
    enc["weight"] = rng.random((n, A), dtype=np.float32) * 1000
    enc["payoff"] = rng.standard_normal((n, A), dtype=np.float32)
    enc["visits"] = rng.integers(0, 1000, (n, A), dtype=np.uint32)
    return past, present, choices, enc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cap-log2", type=int, default=24)
    ap.add_argument("--queries", type=int, default=1 << 22)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--merge-kernel-stats")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "nlhe_policy_rate.json"))
    args = ap.parse_args()
    if args.merge_kernel_stats:
        return merge_kernel_stats(args.merge_kernel_stats, args.out)

    import ctypes as C

    import numpy as np
    import torch

    import nlhe_policy_model as PM
    from robopoker_amd import _lib
    from robopoker_amd.nlhe import A, ENC_DTYPE, NlheSolver

    if not torch.cuda.is_available():
        raise SystemExit("nlhe_policy_rate.py measures on the GPU: no device visible")
    rng = np.random.default_rng(2026)
    n_keys, nq = 1 << (args.cap_log2 - 1), args.queries
    past, present, choices, enc = synthetic_table(rng, n_keys)
    s = NlheSolver(cap_log2=args.cap_log2, batch=1, seed=1)
    t0 = time.perf_counter()
    s.load(past, present, choices, enc, epoch=1)
    load_s = time.perf_counter() - t0
    say(f"loaded {n_keys} keys in {load_s:.1f} s")
    pick = rng.integers(0, n_keys, nq)
    absent = rng.random(nq) < 0.1
    q = (past[pick], np.where(absent, present[pick] ^ np.uint32(1 << 16), present[pick]).astype(np.uint32), choices[pick])
    dev = torch.device("cuda", 0)
    dq = [torch.from_numpy(q[0].view(np.int64)).to(dev), torch.from_numpy(q[1].view(np.int32)).to(dev), torch.from_numpy(q[2].view(np.int64)).to(dev)]
    o_pol = torch.empty((nq, A), dtype=torch.float32, device=dev)
    o_edges = torch.empty((nq, A), dtype=torch.uint8, device=dev)
    o_nact, o_found = torch.empty(nq, dtype=torch.uint8, device=dev), torch.empty(nq, dtype=torch.uint8, device=dev)
    o_enc = torch.empty((nq, A, 16), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(dev)
    s.set_stream(st.cuda_stream)
    lib, p = s._lib, lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def launch(what, shape):
        os.environ["RP_NLHE_QUERY_SHAPE"] = shape
        if what == "memory":
            _lib.check(lib.rp_nlhe_memory_device(s._h, nq, p(dq[0]), p(dq[1]), p(dq[2]), p(o_enc), p(o_nact), p(o_found)))
        else:
            _lib.check(lib.rp_nlhe_policy_device(s._h, _lib.DIST[what], nq, p(dq[0]), p(dq[1]), p(dq[2]), p(o_pol), p(o_edges), p(o_nact), p(o_found)))

    def window(what, shape, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(st):
            e0.record()
            for _ in range(launches):
                launch(what, shape)
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / launches

    cases = [(k, sh) for k in ("iterated", "averaged", "sampling") for sh in ("group", "lane")] + [("memory", "group")]
    for what, shape in cases:  # warm-up of every kernel the timed windows use
        window(what, shape, 2)
    if args.profile_run:
        for what, shape in cases:
            window(what, shape, 5)
        s.sync()
        return
    # the answers of the two shapes at the timed size, and a sample against the model
    same = {}
    sample = np.arange(0, nq, max(1, nq // 4096))
    hp = s.hp
    for kind in ("iterated", "averaged", "sampling"):
        window(kind, "group", 1)
        g = o_pol.clone()
        window(kind, "lane", 1)
        same[kind] = bool(torch.equal(g.view(torch.int32), o_pol.view(torch.int32)))
        want = PM.policy_rows(kind, q[2][sample], enc[pick[sample]], ~absent[sample], temperature=hp.temperature, smoothing=hp.smoothing,
                              curiosity=hp.curiosity)
        same[kind + "_model_sample"] = bool(np.array_equal(g[torch.from_numpy(sample).to(dev)].cpu().numpy().view(np.uint32), want.view(np.uint32)))
    times = {f"{w}/{sh}": [] for w, sh in cases}
    for _ in range(args.rounds):
        for what, shape in cases:
            times[f"{what}/{shape}"].append(window(what, shape, args.launches))
    out = {"device": torch.cuda.get_device_name(0), "cap_log2": args.cap_log2, "keys_loaded": n_keys, "queries": nq, "absent_fraction": float(absent.mean()),
           "launches_per_window": args.launches, "rounds": args.rounds, "load_s": load_s, "hbm_peak_bytes_per_s": HBM_PEAK,
           "shapes_bit_identical": same, "timing": "device events around `launches` launches on one stream, per-launch mean; median of the rounds",
           "results": {}}
    for key, ts in times.items():
        what = key.split("/")[0]
        med = float(np.median(ts))
        bytes_q = KEY_BYTES + SLOT_BYTES + ROW_BYTES[what] + OUT_BYTES[what]
        out["results"][key] = {"seconds_per_launch_rounds": ts, "seconds_per_launch": med, "queries_per_s": nq / med, "algorithmic_bytes_per_query": bytes_q,
                               "algorithmic_bytes_per_s": nq * bytes_q / med, "fraction_of_hbm_peak": nq * bytes_q / med / HBM_PEAK}
        say(f"{key}: {med * 1e3:.3f} ms per launch, {nq / med / 1e9:.3f} G queries/s")
    # the route that existed before: the whole table to the host, then the model there (the join of queries to exported keys not counted)
    s.sync()
    t0 = time.perf_counter()
    xp = s.export()
    export_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    PM.policy_rows("averaged", xp[2], xp[3], np.ones(xp[2].size, bool))
    model_s = time.perf_counter() - t0
    out["export_route"] = {"export_s": export_s, "numpy_model_averaged_s": model_s, "infosets": int(xp[0].size),
                           "note": "rp_nlhe_export of the table + the numpy model over every exported infoset; joining queries to keys is extra"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps({k: v["queries_per_s"] for k, v in out["results"].items()}))


if __name__ == "__main__":
    main()

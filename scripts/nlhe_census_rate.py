#!/usr/bin/env python3
"""Time of the blueprint census (rp_nlhe_table_census, csrc/nlmc_census.hpp) by table size, against the only route the parent commit
has to the same numbers: rp_nlhe_export of every slot and row to the host, then a host fold.

Tables: 2^cap slots for every cap of --caps, filled by rp_nlhe_import with min(slots / 2, --rows-max) random infosets (streets 0..3,
2 to 6 actions of the raise grid).  The import goes through host arrays — 164 bytes per infoset here, a 32-byte slot per slot in the
library — so the default stops at 2^27 slots, half full: 11 GB of keys and rows on the host.  The card holds a table of 2^30 slots;
a table past the row limit is measured at the load the limit leaves, which is recorded.

  census   rp_nlhe_table_census, host form (stage, two launches, 20 800 bytes back, synchronise): --runs runs after a warm-up, a host
           clock around the call; median, min, max.  Bytes touched = 32 B x slots + 144 B x ready slots; the fraction of 8 TB/s.
  export   rp_nlhe_export of the same table (one run after a warm-up at caps up to --export-cap): the parent's route moves every slot
           and every ready row to the host; then tests/nlhe_census_model.py folds them — timed on the first --model-infosets infosets
           and scaled to the table, which is recorded as such.
  kernels  VGPR / LDS / scratch of the two kernels (scripts/kernel_resources.py over csrc/nlmc_census.hpp).

    nlhe_census_rate.py [--caps 20,24,27] [--rows-max 67108864] [--runs 5] [--export-cap 27] [--out profiles/nlhe_census_rate.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
say = lambda m: print(m, file=sys.stderr, flush=True)  # noqa: E731
HBM_BYTES_PER_S = 8e12


def kernel_resources():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "census.hip")
        open(src, "w").write('#include "%s"\n' % os.path.join(R, "robopoker_amd", "csrc", "nlmc_census.hpp"))
        text = subprocess.run([sys.executable, os.path.join(R, "scripts", "kernel_resources.py"), src], capture_output=True, text=True).stdout
    out = {}
    for line in text.splitlines():
        f = line.split()
        if f and f[0].startswith("rp::k_nl_census"):
            out[f[0]] = dict(zip(("vgpr", "agpr", "scratch_bytes", "lds_bytes", "occupancy", "vgpr_spill"), map(int, f[1:7])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--caps", default="20,24,27")
    ap.add_argument("--rows-max", type=int, default=1 << 26)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--export-cap", type=int, default=27)
    ap.add_argument("--model-infosets", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(R, "profiles", "nlhe_census_rate.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import nlhe_census_model as CM
    from robopoker_amd.nlhe import A, ENC_DTYPE, NlheSolver, census_stats

    if not torch.cuda.is_available():
        raise SystemExit("nlhe_census_rate.py measures on the GPU: no device visible")
    rng = np.random.default_rng(2026)
    out = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "hbm_bytes_per_s": HBM_BYTES_PER_S,
           "timing": "host clock around calls that end in a device synchronise; a warm-up, then the runs; median / min / max",
           "kernels": kernel_resources(), "tables": {}}
    say(f"kernels: {out['kernels']}")
    # choices of 2..6 actions: raises of the grid, then shove, call, fold
    paths = []
    for n in range(2, 7):
        codes = list(range(10, 10 + n - 3)) + [5, 4, 2] if n >= 3 else [4, 2]
        paths.append(sum(c << (5 * a) for a, c in enumerate(codes)))
    paths = np.array(paths, np.uint64)

    for cap in [int(c) for c in args.caps.split(",")]:
        slots = 1 << cap
        n = min(slots // 2, args.rows_max)
        past = rng.integers(0, 1 << 63, n, dtype=np.uint64)
        present = (rng.integers(0, 4, n, dtype=np.uint32) << 8) | rng.integers(0, 256, n, dtype=np.uint32)
        choices = paths[rng.integers(0, paths.size, n)]
        enc = np.zeros((n, A), dtype=ENC_DTYPE)
        enc["weight"], enc["regret"] = rng.random((n, A), dtype=np.float32) * 1000, rng.standard_normal((n, A), dtype=np.float32) * 100
        enc["payoff"], enc["visits"] = rng.standard_normal((n, A), dtype=np.float32), rng.integers(0, 1 << 20, (n, A), dtype=np.uint32)
        s = NlheSolver(cap_log2=cap, batch=1, seed=1)
        t0 = time.perf_counter()
        s.load(past, present, choices, enc, epoch=1)
        load_s = time.perf_counter() - t0
        ready = s.counters()[2]
        say(f"cap {cap}: {ready} infosets loaded in {load_s:.1f} s (load {ready / slots:.4f})")
        rec = s.table_census()  # warm-up: allocates the scratch
        assert int(rec["infosets"].sum()) == ready and census_stats(rec)["edges"] == int(CM.PM.nch_rows(choices).sum())
        ts = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            s.table_census()
            ts.append(time.perf_counter() - t0)
        med = float(np.median(ts))
        touched = 32 * slots + 144 * ready
        res = {"slots": slots, "infosets": int(ready), "load": ready / slots, "import_s": load_s, "census_seconds": ts, "census_median_s": med,
               "census_min_s": min(ts), "census_max_s": max(ts), "bytes_touched": touched, "bytes_per_s": touched / med,
               "fraction_of_hbm": touched / med / HBM_BYTES_PER_S, "segments": max(1, slots // CM.SEGMENT)}
        say(f"cap {cap}: census {med * 1e3:.3f} ms [{min(ts) * 1e3:.3f}, {max(ts) * 1e3:.3f}], {touched / 1e9:.2f} GB touched, "
            f"{touched / med / 1e9:.1f} GB/s = {res['fraction_of_hbm'] * 100:.1f} % of 8 TB/s")
        if cap <= args.export_cap:
            s.export()  # warm-up
            t0 = time.perf_counter()
            ex = s.export()
            export_s = time.perf_counter() - t0
            m = min(args.model_infosets, ready)
            t0 = time.perf_counter()
            CM.census(np.arange(m), ex[0][:m], ex[1][:m], ex[2][:m], ex[3][:m], epoch=1, slots=slots)
            model_s = (time.perf_counter() - t0) * ready / m
            res.update(export_s=export_s, export_bytes=32 * slots + (20 + 144) * ready, host_fold_s_scaled=model_s, host_fold_timed_on_infosets=m,
                       parent_route_s=export_s + model_s, census_speedup_over_export_alone=export_s / med,
                       census_speedup_over_parent_route=(export_s + model_s) / med)
            say(f"cap {cap}: export {export_s:.3f} s, host fold (scaled from {m} infosets) {model_s:.1f} s: the census is "
                f"{export_s / med:.0f}x the export alone, {(export_s + model_s) / med:.0f}x the route")
        out["tables"][str(cap)] = res
        s.close()
        del s, past, present, choices, enc
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps({c: {"census_ms": r["census_median_s"] * 1e3, "fraction_of_hbm": r["fraction_of_hbm"], "load": r["load"]}
                      for c, r in out["tables"].items()}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Rate of matches played on the device (rp_nlhe_match, csrc/nlmc_match.hpp): hands/s of the host form by batch and agent pairing.

Workload: heads-up hands from the deal to the settlement, stacks 200, alternating dealer, every hand distinct (hand i of a call is
hand id i of the seed).  The blueprint is defined key by key by a hash, as scripts/nlhe_aivat_rate.py defines its own (half of the
infosets have a row; weights in (0, 1000), payoffs in (-100, 100)); the table has 2^cap_log2 slots and holds the rows that
`--model-hands` hands played by the host model ask for, plus synthetic filler up to a quarter of it.  One table serves both seats.

  match      rp_nlhe_match, host form: nothing up, one launch per 2^20 hands, 192 + 4 bytes per hand back; the pairings
             blueprint-blueprint, dirac-blueprint, fish-blueprint.
  playouts   rp_nlhe_playouts for the same number of games: the rules engine alone, no bucket, no probe, no record.
  model      the only route the parent commit has: the table played in Python over the CPU oracle (tests/nlhe_match_model.py).
  pipeline   match_device -> aivat_device -> sync against the same two calls through host memory (match, then aivat).
Timed with a host clock around calls that end in a device synchronise, `--runs` runs each after a warm-up; median, min and max.

    nlhe_match_rate.py [--cap-log2 20] [--runs 5] [--model-hands 128] [--batches 1,64,4096,262144] [--out profiles/nlhe_match_rate.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cap-log2", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--model-hands", type=int, default=128)
    ap.add_argument("--batches", default="1,64,4096,262144")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "nlhe_match_rate.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import nlhe_match_model as MM
    import nlhe_policy_model as PM
    from robopoker_amd import nlhe
    from robopoker_amd.nlhe import A, ENC_DTYPE, NlheSolver

    if not torch.cuda.is_available():
        raise SystemExit("nlhe_match_rate.py measures on the GPU: no device visible")
    rng = np.random.default_rng(2026)
    F = np.float32
    SEED = 2026
    PAIRINGS = (("blueprint", "blueprint"), ("dirac", "blueprint"), ("fish", "blueprint"))

    class Blueprint:
        """rows by a hash of the key, remembered as asked; the model reads the weights"""

        def __init__(self):
            self.rows = {}

        def get(self, key):
            if key not in self.rows:
                h = PM.key_hash(key[0] ^ 0xA17A7, key[2], key[1])
                row = None
                if h % 2 == 0:
                    g = np.random.default_rng(h)
                    row = ((g.random(A, dtype=F) * 1000 + 1).astype(F), (g.random(A, dtype=F) * 200 - 100).astype(F))
                self.rows[key] = row
            return None if self.rows[key] is None else self.rows[key][0]

    # ---- the host model: its hands define the rows of the table, and its time is the parent commit's route
    bp = Blueprint()
    model, model_s = {}, {}
    for pair in PAIRINGS:
        t0 = time.perf_counter()
        model[pair] = MM.match(args.model_hands, MM.Args(seed=SEED, agents=pair), (bp, bp))
        model_s[pair] = time.perf_counter() - t0
        say(f"model {pair}: {args.model_hands} hands in {model_s[pair]:.2f} s")

    own = [k for k, r in bp.rows.items() if r is not None]
    n_fill = max(0, (1 << (args.cap_log2 - 2)) - len(own))
    past = np.concatenate([np.array([k[0] for k in own], np.uint64), rng.integers(1 << 61, 1 << 63, n_fill, dtype=np.uint64)])
    present = np.concatenate([np.array([k[1] for k in own], np.uint32), rng.integers(0, 1 << 10, n_fill, dtype=np.uint32)])
    choices = np.concatenate([np.array([k[2] for k in own], np.uint64), np.full(n_fill, 2 | 4 << 5 | 5 << 10, np.uint64)])
    enc = np.zeros((past.size, A), dtype=ENC_DTYPE)
    enc["weight"], enc["payoff"] = rng.random((past.size, A), dtype=F) * 1000, rng.random((past.size, A), dtype=F)
    enc["weight"][: len(own)] = np.stack([bp.rows[k][0] for k in own])
    enc["payoff"][: len(own)] = np.stack([bp.rows[k][1] for k in own])
    s = NlheSolver(cap_log2=args.cap_log2, batch=1, seed=1)
    s.load(past, present, choices, enc, epoch=1)
    say(f"table: 2^{args.cap_log2} slots, {past.size} rows loaded ({len(own)} of them infosets the model's hands ask for)")

    def timed(fn):
        fn()  # warm-up
        ts = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return ts

    def figures(ts, n):
        med = float(np.median(ts))
        return {"seconds": ts, "median_s": med, "min_s": min(ts), "max_s": max(ts), "hands_per_s": n / med}

    out = {"device": torch.cuda.get_device_name(0), "cap_log2": args.cap_log2, "rows_loaded": int(past.size), "runs": args.runs,
           "timing": "host clock around calls that end in a device synchronise; a warm-up, then the runs; median / min / max",
           "host_model": {"-".join(p): {"hands": args.model_hands, "seconds": model_s[p], "hands_per_s": args.model_hands / model_s[p]}
                          for p in PAIRINGS},
           "results": {}}
    for n in [int(b) for b in args.batches.split(",")]:
        res = {}
        for pair in PAIRINGS:
            kw = dict(seed=SEED, agents=pair)
            got = s.match(n, **kw)
            m = min(n, args.model_hands)  # the first hands of the batch are the model's hands
            want = model[pair][:m]
            same = all(got["status"][i] == w["status"] and got["won"][i] == w["won"] and got["rejected"][i] == w["rejected"]
                       and got["hands"]["n_plays"][i] == w["n_plays"] for i, w in enumerate(want))
            r = figures(timed(lambda: s.match(n, **kw)), n)
            r["model_agrees_on_the_first_hands"] = bool(same)
            r["mean_plays"] = float(got["hands"]["n_plays"].mean())
            r["mean_streets"] = float((got["hands"]["draws"] != 0).sum(axis=1).mean())
            r["status_counts"] = np.bincount(got["status"], minlength=8).tolist()
            r["rejected_per_hand"] = float(got["rejected"].mean())
            res["-".join(pair)] = r
            say(f"batch {n} {pair}: {r['median_s'] * 1e3:.3f} ms [{r['min_s'] * 1e3:.3f}, {r['max_s'] * 1e3:.3f}], {r['hands_per_s']:.3g} hands/s, "
                f"{r['mean_plays']:.2f} plays, {r['mean_streets']:.2f} streets, model agrees: {same}")
        res["playouts"] = figures(timed(lambda: (nlhe.playouts(2, n, SEED), torch.cuda.synchronize())), n)
        say(f"batch {n} playouts: {res['playouts']['median_s'] * 1e3:.3f} ms")
        out["results"][str(n)] = res

    # ---- the pipeline at the largest batch: device tensors all the way against the same two calls through host memory
    n = max(int(b) for b in args.batches.split(","))
    kw = dict(seed=SEED, dealer=0, board_mode=1)

    def on_device():
        dev = s.match_device(n, **kw)
        a = s.aivat_device(dev["hands"])
        s.sync()
        return dev, a

    def through_host():
        h = s.match(n, **kw)
        return h, s.aivat(h["hands"])

    (dev, da), (host, ha) = on_device(), through_host()
    same = (np.array_equal(dev["won"].cpu().numpy(), host["won"])
            and np.array_equal(da["total"].cpu().numpy().view(np.uint32), ha["total"].view(np.uint32))
            and np.array_equal(da["status"].cpu().numpy(), ha["status"]))
    out["pipeline"] = {"hands": n, "device": figures(timed(on_device), n), "through_host": figures(timed(through_host), n),
                       "same_answers": bool(same), "aivat_status_counts": np.bincount(ha["status"], minlength=12).tolist()}
    say(f"pipeline {n}: device {out['pipeline']['device']['median_s'] * 1e3:.2f} ms, through host {out['pipeline']['through_host']['median_s'] * 1e3:.2f} ms, same: {same}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps({b: {k: v["hands_per_s"] for k, v in r.items()} for b, r in out["results"].items()}))


if __name__ == "__main__":
    main()

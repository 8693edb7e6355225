#!/usr/bin/env python3
"""Rate of translating played hands to recalls on the device (rp_nlhe_translate, csrc/nlmc_translate.hpp): hands/s of the _device
form for each of the three translations, beside the time of the match that played the same hands.

Workload: `--hands` (2^20) heads-up hands of a blueprint-vs-fish rp_nlhe_match_device (stacks 200, alternating dealer, every hand
distinct) on a table trained `--steps` steps at batch 128 — the fish raises the minimum, so most raises are off the grid.  The hands
stay in device memory: translate_device reads the match's records where the match wrote them.  Every hand is translated whole
(upto = n_plays, pov = the hero).

Timed with a host clock around calls that end in a device synchronise, `--runs` runs each after a warm-up, the four calls taken in
turn within every run; median, min and max.  The expectation stated beside the numbers: translating takes no longer than playing the
same hands, since it is the same replay without table probes.

    nlhe_translate_rate.py [--hands 1048576] [--steps 3] [--runs 7] [--out profiles/nlhe_translate_rate.json]
"""
import argparse
import json
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
say = lambda m: print(m, file=sys.stderr, flush=True)  # noqa: E731
KINDS = ("snap", "harmonic", "phargmax")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hands", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(R, "profiles", "nlhe_translate_rate.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from robopoker_amd.nlhe import AIVAT_DTYPE, NlheSolver

    if not torch.cuda.is_available():
        raise SystemExit("nlhe_translate_rate.py measures on the GPU: no device visible")
    n = args.hands
    s = NlheSolver(cap_log2=18, batch=128, seed=5, sampling="pluribus")
    for _ in range(args.steps):
        s.step()
    kw = dict(agents=("blueprint", "fish"), seed=2026)

    def play():
        dev = s.match_device(n, **kw)
        s.sync()
        return dev

    hands = play()["hands"]

    def translate(kind):
        out = s.translate_device(hands, kind, seed=2026)
        s.sync()
        return out

    calls = {"match": play, **{k: (lambda k=k: translate(k)) for k in KINDS}}
    for fn in calls.values():  # warm-up: every code object loaded, every output size allocated once
        fn()
    seconds = {name: [] for name in calls}
    for _ in range(args.runs):
        for name, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            seconds[name].append(time.perf_counter() - t0)

    def figures(ts):
        med = float(np.median(ts))
        return {"seconds": ts, "median_s": med, "min_s": min(ts), "max_s": max(ts), "hands_per_s": n / med}

    records = hands.cpu().numpy().reshape(-1).view(AIVAT_DTYPE)
    got = {k: translate(k) for k in KINDS}
    edges = {k: got[k]["play_edges"].cpu().numpy() for k in KINDS}
    raises = records["kind"] == 4
    out = {"device": torch.cuda.get_device_name(0), "hands": n, "train_steps": args.steps, "runs": args.runs,
           "timing": "host clock around calls that end in a device synchronise; a warm-up, then the runs, the calls in turn; median / min / max",
           "bytes_per_hand": {"in": 192, "out": 88 + 48 + 8 + 4 + 8 + 1 + 1},
           "mean_plays": float(records["n_plays"].mean()), "mean_streets": float((records["draws"] != 0).sum(axis=1).mean()),
           "raises_per_hand": float(raises.sum() / n),
           "status_counts": {k: np.bincount(got[k]["status"].cpu().numpy(), minlength=8).tolist() for k in KINDS},
           "raises_translated_differently_from_snap": {k: float((edges[k] != edges["snap"])[raises].mean()) for k in KINDS[1:]},
           "match_device": figures(seconds["match"]), "translate_device": {k: figures(seconds[k]) for k in KINDS},
           "expectation": "translating takes no longer than playing the same hands: the same replay without table probes"}
    slowest = max(out["translate_device"][k]["median_s"] for k in KINDS)
    out["expectation_holds"] = bool(slowest <= out["match_device"]["median_s"])
    out["effective_bytes_per_s"] = {k: n * (192 + 158) / out["translate_device"][k]["median_s"] for k in KINDS}
    for name in calls:
        f = out["match_device"] if name == "match" else out["translate_device"][name]
        say(f"{name}: {f['median_s'] * 1e3:.3f} ms [{f['min_s'] * 1e3:.3f}, {f['max_s'] * 1e3:.3f}], {f['hands_per_s']:.4g} hands/s")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps({"match_device_hands_per_s": out["match_device"]["hands_per_s"], "expectation_holds": out["expectation_holds"],
                      **{k: out["translate_device"][k]["hands_per_s"] for k in KINDS}}))


if __name__ == "__main__":
    main()

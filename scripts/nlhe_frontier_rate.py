#!/usr/bin/env python3
"""Rate of the frontier payoff query (rp_nlhe_frontier_payoffs, csrc/nlmc_frontier.hpp) against the playout kernel that has the same
shape without the lookups.

Workload: chance frontiers after open and call (the reference's case: a depth-limited leaf before the flop is dealt), prefix = the
history, holes drawn from a seed, 64 distinct frontiers (larger batches repeat them), rollouts = 16, bias = 5: 256 games per frontier.
The table is a blueprint trained for `--train-steps` steps of `--train-batch` trees with the hash encoder.

  frontier  rp_nlhe_frontier_payoffs_device: the records already in device memory, one launch, timed from the call to rp_nlhe_sync.
  playouts  rp_nlhe_playouts at the same number of games (2 seats): one lane per game from the preflop root, uniform picks, no bucket,
            no probe, no policy; it synchronises itself.
Both are timed with a host clock, alternating, `--runs` runs each after a warm-up; median, min and max are reported.  The games differ
in length (a playout starts a street earlier and picks uniformly), so the two are compared in rollout-STEPS per second: the playout
kernel reports its steps; the frontier kernel does not, and its mean steps per rollout are counted by the model
(tests/nlhe_rollout_model.py) over a sample of the same frontiers against the exported table.

    nlhe_frontier_rate.py [--cap-log2 20] [--runs 5] [--batches 1,64,4096] [--out profiles/nlhe_frontier_rate.json]
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

# k_nl_frontier as hipcc -Rpass-analysis=kernel-resource-usage reports it for gfx950 (csrc/Makefile's flags)
STATIC = {"vgprs": 110, "agprs": 0, "sgprs": 106, "sgpr_spills": 30, "vgpr_spills": 0, "scratch_bytes_per_lane": 0, "lds_bytes_per_block": 8304,
          "occupancy_waves_per_simd": 4, "block": 256}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cap-log2", type=int, default=20)
    ap.add_argument("--train-steps", type=int, default=4)
    ap.add_argument("--train-batch", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--rollouts", type=int, default=16)
    ap.add_argument("--bias", type=float, default=5.0)
    ap.add_argument("--sample", type=int, default=4, help="frontiers whose rollouts the model replays to count steps")
    ap.add_argument("--batches", default="1,64,4096")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "nlhe_frontier_rate.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import nlhe_rollout_model as FM
    import oracle_nlhe as ON
    from robopoker_amd.nlhe import Frontier, NlheSolver, playouts

    if not torch.cuda.is_available():
        raise SystemExit("nlhe_frontier_rate.py measures on the GPU: no device visible")
    rng = np.random.default_rng(2026)
    history = [ON.Open(2), ON.E_CALL]
    frontiers = []
    for _ in range(args.distinct):
        c = [int(x) for x in rng.permutation(52)[:4]]
        frontiers.append(Frontier((1 << c[0] | 1 << c[1], 1 << c[2] | 1 << c[3]), 0, edges=history, prefix=history))

    s = NlheSolver(cap_log2=args.cap_log2, batch=args.train_batch, seed=1)
    for _ in range(args.train_steps):
        s.step("composed")
    keys = s.counters()[2]
    say(f"table: 2^{args.cap_log2} rows, {keys} infosets after {args.train_steps} steps of {args.train_batch} trees")

    # ---- mean steps per rollout, and the model's bits for the sampled frontiers
    xp = s.export()
    rows = {(int(p), int(q), int(c)): xp[3]["weight"][i] for i, (p, q, c) in enumerate(zip(*xp[:3]))}
    t0 = time.perf_counter()
    steps, games, found = 0, 0, 0
    sample = frontiers[: args.sample]
    got = s.frontier_payoffs(sample, args.bias, args.rollouts, 7, 0, return_won=True)
    same = True
    for i, f in enumerate(sample):
        game = FM.frontier_game(f)
        for cell in range(16):
            for r in range(args.rollouts):
                used, stream = [], FM.Stream(7, FM.rollout_id(0, i, cell >> 2, cell & 3, args.rollouts, r))
                won = FM.rollout(game, f.prefix, 0, cell >> 2, cell & 3, rows, args.bias, stream, used)
                dealt = stream.c - len(used)  # cards: 3 to the flop, then 1 and 1
                steps += len(used) + (0 if dealt == 0 else dealt - 2)
                found += sum(1 for _, hit, _ in used if hit)
                games += 1
                same = same and won == got[2][i, cell, r]
    decisions_found = found
    mean_steps = steps / games
    say(f"model: {games} rollouts replayed in {time.perf_counter() - t0:.1f} s, {mean_steps:.2f} steps each, same bits as the device: {same}")

    out = {"device": torch.cuda.get_device_name(0), "cap_log2": args.cap_log2, "infosets": int(keys), "train_steps": args.train_steps,
           "train_batch": args.train_batch, "rollouts": args.rollouts, "bias": args.bias, "distinct_frontiers": args.distinct, "runs": args.runs,
           "static_resources_k_nl_frontier": STATIC,
           "steps_per_rollout": {"mean": mean_steps, "rollouts_replayed": games, "decisions_with_a_row": decisions_found,
                                 "how": "tests/nlhe_rollout_model.py over the first frontiers against the exported table; steps = decisions + streets dealt"},
           "model_bits_equal_on_the_sample": bool(same),
           "timing": "host clock; frontier: _device form, from the call to rp_nlhe_sync; playouts: the call (it synchronises); alternating; median / min / max",
           "results": {}}
    for n in [int(b) for b in args.batches.split(",")]:
        idx = np.arange(n) % args.distinct
        rec = torch.from_numpy(Frontier.pack([frontiers[i] for i in idx]).view(np.uint8).copy()).to("cuda")
        n_games = n * 16 * args.rollouts

        def frontier():
            t0 = time.perf_counter()
            ans = s.frontier_payoffs_device(rec, args.bias, args.rollouts, 7, 0)
            s.sync()
            return time.perf_counter() - t0, ans

        def playout():
            t0 = time.perf_counter()
            ans = playouts(2, n_games, 7)
            return time.perf_counter() - t0, ans

        _, fa = frontier()  # warm-up of both
        _, pa = playout()
        assert not fa[1].cpu().numpy().any(), "a frontier of the workload was refused"
        play_steps = int(pa[2].cpu().numpy().astype(np.int64).sum())
        tf, tp = [], []
        for _ in range(args.runs):
            tf.append(frontier()[0])
            tp.append(playout()[0])
        mf, mp = float(np.median(tf)), float(np.median(tp))
        res = {"frontier": {"seconds": tf, "median_s": mf, "min_s": min(tf), "max_s": max(tf), "frontiers_per_s": n / mf,
                            "rollouts_per_s": n_games / mf, "rollout_steps_per_s": n_games * mean_steps / mf},
               "playouts": {"seconds": tp, "median_s": mp, "min_s": min(tp), "max_s": max(tp), "games": n_games, "steps": play_steps,
                            "games_per_s": n_games / mp, "steps_per_s": play_steps / mp}}
        res["steps_per_s_ratio_frontier_over_playouts"] = res["frontier"]["rollout_steps_per_s"] / res["playouts"]["steps_per_s"]
        out["results"][str(n)] = res
        say(f"batch {n}: frontier {mf * 1e3:.3f} ms [{min(tf) * 1e3:.3f}, {max(tf) * 1e3:.3f}] = {n_games / mf:.3g} rollouts/s; playouts "
            f"{mp * 1e3:.3f} ms [{min(tp) * 1e3:.3f}, {max(tp) * 1e3:.3f}]; steps/s ratio {res['steps_per_s_ratio_frontier_over_playouts']:.3f}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps({b: {"frontiers_per_s": r["frontier"]["frontiers_per_s"], "rollouts_per_s": r["frontier"]["rollouts_per_s"],
                          "steps_ratio": r["steps_per_s_ratio_frontier_over_playouts"]} for b, r in out["results"].items()}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""How large a safe subgame solve gets: the model (tests/nlhe_subgame_model.py, no GPU) run for `--iterations` iterations over the flop
entries of scripts/nlhe_subgame_rate.py, at RP_NLHE_SUBGAME_ORIGIN_NONE and at origin = street - 1, recording the largest tree (nodes,
infosets with children, frontiers) and the largest local profile (rows).  DESIGN.md §3i takes the caps of k_nl_subgame from this.

The blueprint is tests/nlhe_depth_model.Blueprint (decided key by key, about half of the keys present): the table the rate script trains
lives on the device.  The belief spreads the candidate holes evenly over the four worlds with equal weights, which is the widest split
of a profile a belief can cause.  One rollout per cell: the counts depend on the payoffs only through the sampled branches.

    nlhe_subgame_caps.py [--iterations 128] [--distinct 64] [--out profiles/nlhe_subgame_caps.json]
"""
import argparse
import json
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))


def flop_entries(distinct):
    """the rate scripts' entries: open, call, the flop, seat 0 to act; holes and flops from one seeded permutation each"""
    import numpy as np

    import oracle_nlhe as ON
    from robopoker_amd.nlhe import Frontier

    rng = np.random.default_rng(2026)
    to_flop = [ON.Open(2), ON.E_CALL, ON.E_DRAW]
    entries = []
    for _ in range(distinct):
        c = [int(x) for x in rng.permutation(52)[:7]]
        holes, flop = (1 << c[0] | 1 << c[1], 1 << c[2] | 1 << c[3]), 1 << c[4] | 1 << c[5] | 1 << c[6]
        entries.append(Frontier(holes, 0, [flop], to_flop))
    return entries


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=128)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(R, "profiles", "nlhe_subgame_caps.json"))
    args = ap.parse_args()

    import numpy as np

    import nlhe_depth_model as DM
    import nlhe_subgame_model as SM

    hole_world = (np.arange(1326) % 4).astype(np.uint8)
    weights = np.full(4, 0.25, np.float32)
    out = {"iterations": args.iterations, "entries": args.distinct, "blueprint": "tests/nlhe_depth_model.Blueprint", "rollouts": 1,
           "belief": "candidate j in world j % 4, equal weights", "caps": {"nodes": DM.MAX_NODES, "infosets": DM.MAX_INFOS,
                                                                          "frontiers": DM.MAX_FRONTIERS, "rows": SM.MAX_ROWS}}
    bp = DM.Blueprint()
    for name, origin in (("origin_none", None), ("street_minus_1", 0)):
        top = {"nodes": 0, "infosets": 0, "frontiers": 0, "rows": 0, "rows_depth_model": 0}
        statuses = {}
        for i, entry in enumerate(flop_entries(args.distinct)):
            keep = []
            got = SM.solve(entry, hole_world, weights, origin, bp, i, args.iterations, keep=keep, rollouts=1, bp_epoch=3, seed=7)
            statuses[got["status"]] = statuses.get(got["status"], 0) + 1
            s = keep[0]
            per_tree = {}
            for t, _, info, _, _ in s.spans:
                per_tree[t] = per_tree.get(t, 0) + (info[0] != "chance")
            top["nodes"] = max([top["nodes"]] + [len(tree) for tree in s.trees])
            top["infosets"] = max([top["infosets"]] + list(per_tree.values()))
            top["frontiers"] = max([top["frontiers"]] + [sum(n.frontier is not None for n in tree) for tree in s.trees])
            top["rows"] = max(top["rows"], len(s.profile.local))
            # the same entry under the depth solve, its own hole kept: what the tag adds
            depth = DM.solve(entry, origin, bp, i, args.iterations, rollouts=1, bp_epoch=3, seed=7)  # None: the entry's street, no frontier
            top["rows_depth_model"] = max(top["rows_depth_model"], depth["n_rows"])
            print(f"{name} entry {i}: rows {len(s.profile.local)} (depth solve {depth['n_rows']}), largest so far {top}", file=sys.stderr, flush=True)
        out[name] = dict(top, statuses=statuses)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

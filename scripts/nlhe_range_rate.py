#!/usr/bin/env python3
"""Rate of the fused range query (rp_nlhe_reaches, csrc/nlmc_range.hpp) against the route a caller had before it existed.

Workload: river recalls — a 15-edge history (three streets checked through, a raising war on the river), 990 candidate holes and 6
subject nodes each — at batches 1, 64 and 4 096.  64 distinct recalls (boards and holes drawn from a seed) are keyed on the host;
larger batches repeat them.  The table has 2^cap_log2 rows: half of the infosets these recalls ask for are loaded, the rest up to a
quarter of the table is synthetic filler.

  fused     rp_nlhe_reaches, host form: n recall structs (88 B) up, one launch, count / holes / reach back.
  composed  what the parent commit offers for the same answer: the keys of every (recall, hole, node) built on the host, ONE
            rp_nlhe_policy call (host form: 20 B per key up, 36 B of policy back; edges / n_actions / found not asked for), the column
            of the edge taken picked and multiplied on the host in float32.  The host replay and keying are NOT in the timed window
            (they are done once, with the test oracle through ctypes, and their time is reported on its own): the composed figure is a
            lower bound of that route.
Both are timed with a host clock around calls that end in a device synchronise, alternating, `--runs` runs each after a warm-up of
every shape; median, min and max are reported.  The two answers are compared bit for bit at every batch.

    nlhe_range_rate.py [--cap-log2 20] [--runs 5] [--batches 1,64,4096] [--out profiles/nlhe_range_rate.json]
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
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--batches", default="1,64,4096")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "nlhe_range_rate.json"))
    args = ap.parse_args()

    import ctypes as C

    import numpy as np
    import torch

    import nlhe_policy_model as PM
    import nlhe_range_model as RM
    import oracle_nlhe as ON
    from robopoker_amd import _lib
    from robopoker_amd.nlhe import A, ENC_DTYPE, NlheSolver, Recall

    if not torch.cuda.is_available():
        raise SystemExit("nlhe_range_rate.py measures on the GPU: no device visible")
    rng = np.random.default_rng(2026)
    pot = ON.RaiseOdds(1, 1)
    edges = [ON.Open(2), pot, ON.E_CALL, 1, 3, 3, 1, 3, 3, 1, 3, pot, pot, pot, ON.E_CALL]

    # ---- the distinct recalls and, on the host, what the composed route needs: per recall the candidates, per (candidate, node) a key
    t0 = time.perf_counter()
    recalls, keys, slots, holes_want = [], [], [], []
    for _ in range(args.distinct):
        c = [int(x) for x in rng.permutation(52)[:7]]
        r = Recall(0, 1 << c[0] | 1 << c[1], [1 << c[2] | 1 << c[3] | 1 << c[4], 1 << c[5], 1 << c[6]], edges)
        draws = RM.validate(r)
        street, board, _ = RM.board_of(r, draws)
        cands = RM.hand_iterator(board | r.hole)
        nodes, _ = RM.replay(r, [r.hole, cands[0]], 1, draws)  # the public part of every node: past, choices, street, edge taken
        boards = [0, draws[0], draws[0] | draws[1], board]
        present = np.array([[RM._bucket(k[1] >> 8, h, boards[k[1] >> 8]) for k, _ in nodes] for h in cands], np.uint32)
        keys.append((np.tile(np.array([k[0] for k, _ in nodes], np.uint64), (len(cands), 1)), present,
                     np.tile(np.array([k[2] for k, _ in nodes], np.uint64), (len(cands), 1))))
        slots.append([list(PM.edges(k[2])).index(e) for k, e in nodes])
        recalls.append(r)
        holes_want.append(np.array(cands, np.uint64))
    keying_s = time.perf_counter() - t0
    count, n_nodes = keys[0][0].shape
    assert all(k[0].shape == (count, n_nodes) for k in keys) and count == 990
    say(f"{args.distinct} recalls keyed on the host in {keying_s:.1f} s: {count} holes x {n_nodes} nodes each")

    # ---- the table
    flat = [np.concatenate([k[i].ravel() for k in keys]) for i in range(3)]
    uniq = np.unique(np.stack([flat[0], flat[1].astype(np.uint64), flat[2]], axis=1), axis=0)
    uniq = uniq[rng.random(len(uniq)) < 0.5]
    n_fill = max(0, (1 << (args.cap_log2 - 2)) - len(uniq))
    past = np.concatenate([uniq[:, 0], rng.integers(1 << 40, 1 << 63, n_fill, dtype=np.uint64)])
    present = np.concatenate([uniq[:, 1].astype(np.uint32), rng.integers(0, 1 << 10, n_fill, dtype=np.uint32)])
    choices = np.concatenate([uniq[:, 2], np.full(n_fill, 2 | 4 << 5 | 5 << 10, np.uint64)])
    enc = np.zeros((past.size, A), dtype=ENC_DTYPE)
    enc["weight"] = rng.random((past.size, A), dtype=np.float32) * 1000
    s = NlheSolver(cap_log2=args.cap_log2, batch=1, seed=1)
    s.load(past, present, choices, enc, epoch=1)
    say(f"table: 2^{args.cap_log2} rows, {past.size} loaded ({len(uniq)} of them infosets the recalls ask for)")

    def fused(rec):
        return s.reaches_raw(rec, "opponent")

    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    pol_buf = {}  # the policy array of a batch size, reused across runs as a caller would

    def composed(kp, kq, kc, slot, n):
        pol = pol_buf.setdefault(n, np.zeros((n * count * n_nodes, A), np.float32))
        _lib.check(s._lib.rp_nlhe_policy(s._h, _lib.DIST["averaged"], kp.size, ptr(kp), ptr(kq), ptr(kc), ptr(pol), None, None, None))
        pol = pol.reshape(n, count, n_nodes, A)
        reach = np.ones((n, count), np.float32)
        for k in range(n_nodes):
            reach = reach * np.take_along_axis(pol[:, :, k, :], slot[:, None, k, None], axis=2)[:, :, 0]
        return reach

    out = {"device": torch.cuda.get_device_name(0), "cap_log2": args.cap_log2, "rows_loaded": int(past.size), "distinct_recalls": args.distinct,
           "holes_per_recall": int(count), "subject_nodes_per_recall": int(n_nodes), "runs": args.runs,
           "host_keying": {"seconds_for_the_distinct_recalls": keying_s, "how": "CPU oracle through ctypes, one public replay per recall and one "
                           "bucket per (hole, street); not in any timed window below"},
           "timing": "host clock around a host-form call that ends in a device synchronise; fused and composed alternate; median / min / max of the runs",
           "results": {}}
    for n in [int(b) for b in args.batches.split(",")]:
        idx = np.arange(n) % args.distinct
        rec = Recall.pack([recalls[i] for i in idx])
        kp, kq, kc = (np.concatenate([keys[i][f].ravel() for i in idx]) for f in range(3))
        slot = np.array([slots[i] for i in idx], np.int64)
        f0, c0 = fused(rec), composed(kp, kq, kc, slot, n)  # warm-up of both shapes, and the comparison of their answers
        same = bool((f0["count"] == count).all() and not f0["status"].any()
                    and np.array_equal(f0["reach"][:, :count].view(np.uint32), c0.view(np.uint32))
                    and all(np.array_equal(f0["holes"][j, :count], holes_want[i]) for j, i in enumerate(idx[: args.distinct])))
        tf, tc = [], []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            fused(rec)
            tf.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            composed(kp, kq, kc, slot, n)
            tc.append(time.perf_counter() - t0)
        res = {}
        for name, ts in (("fused", tf), ("composed_lower_bound", tc)):
            med = float(np.median(ts))
            res[name] = {"seconds": ts, "median_s": med, "min_s": min(ts), "max_s": max(ts), "recalls_per_s": n / med, "hole_reaches_per_s": n * count / med}
        res["bit_identical"] = same
        res["bytes_moved"] = {"fused_up": n * 88, "fused_back": n * (1326 * 12 + 5), "composed_up": n * count * n_nodes * 20, "composed_back": n * count * n_nodes * 36}
        res["fused_faster_beyond_spread"] = bool(max(tf) < min(tc))
        res["speedup_of_medians"] = res["composed_lower_bound"]["median_s"] / res["fused"]["median_s"]
        out["results"][str(n)] = res
        say(f"batch {n}: fused {res['fused']['median_s'] * 1e3:.2f} ms [{min(tf) * 1e3:.2f}, {max(tf) * 1e3:.2f}], composed >= "
            f"{res['composed_lower_bound']['median_s'] * 1e3:.2f} ms [{min(tc) * 1e3:.2f}, {max(tc) * 1e3:.2f}], same bits: {same}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps({b: {"fused_recalls_per_s": r["fused"]["recalls_per_s"], "speedup_of_medians": r["speedup_of_medians"],
                          "bit_identical": r["bit_identical"]} for b, r in out["results"].items()}))


if __name__ == "__main__":
    main()

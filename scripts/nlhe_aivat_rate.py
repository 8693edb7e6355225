#!/usr/bin/env python3
"""Rate of the fused AIVAT evaluation (rp_nlhe_aivat, csrc/nlmc_aivat.hpp) against the route a caller had before it existed.

Workload: heads-up hands generated on the host, once and outside every timed window, by playing the loaded blueprint against itself
(stacks 200, dealer 0, the cards from a seed; at a node without a row, or with zero weight, the play is uniform over the node's
choices).  The blueprint is defined key by key by a hash (half of the infosets have a row; weights in (0, 1000), payoffs in
(-100, 100)); the table has 2^cap_log2 slots and holds the rows the hands ask for plus synthetic filler up to a quarter of it.
`--distinct` hands are generated; larger batches repeat them.  board_mode 1, so that nodes of every street can find their row.

  fused     rp_nlhe_aivat, host form: n hands (192 B) up, one launch per 2^20 hands, 4 floats + 3 bytes per hand back.
  composed  what the parent commit offers for the same answer: the two-game replay on the host (the test model over the CPU oracle),
            which yields every key a hand asks for, rp_nlhe_memory by key (host form, 20 B per key up, 144 B back, at most 2^21 keys
            per call), the folds on the host.  Only the rp_nlhe_memory calls are in the timed window: the figure is a LOWER BOUND of
            that route (the host replay's time for the distinct hands is reported on its own).
Both are timed with a host clock around calls that end in a device synchronise, alternating, `--runs` runs each after a warm-up of
both; median, min and max are reported.  bit_identical: the model, fed the Encounters rp_nlhe_memory answered, gives the fused call's
six outputs and status for every distinct hand, and every repeat in the batch answers as its original.

    nlhe_aivat_rate.py [--cap-log2 20] [--runs 5] [--distinct 128] [--batches 1,64,4096,262144] [--out profiles/nlhe_aivat_rate.json]
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
    ap.add_argument("--distinct", type=int, default=128)
    ap.add_argument("--batches", default="1,64,4096,262144")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "nlhe_aivat_rate.json"))
    args = ap.parse_args()

    import ctypes as C

    import numpy as np
    import torch

    import nlhe_aivat_model as AM
    import nlhe_policy_model as PM
    import nlhe_range_model as RM
    import oracle_nlhe as ON
    from robopoker_amd import _lib
    from robopoker_amd.nlhe import A, ENC_DTYPE, AivatHand, NlheSolver

    if not torch.cuda.is_available():
        raise SystemExit("nlhe_aivat_rate.py measures on the GPU: no device visible")
    rng = np.random.default_rng(2026)
    F = np.float32

    class Blueprint:
        """rows by a hash of the key, remembered as asked"""

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
            return self.rows[key]

    bp = Blueprint()
    o = ON.lib()

    def play():
        c = [int(x) for x in rng.permutation(52)[:9]]
        holes = (1 << c[0] | 1 << c[1], 1 << c[2] | 1 << c[3])
        draws = [1 << c[4] | 1 << c[5] | 1 << c[6], 1 << c[7], 1 << c[8]]
        g, w, plays = AM._start(0, (ON.STACK, ON.STACK), holes), AM.Witness(holes[0], draws), []
        while AM._turn(g) != ON.TERMINAL and len(plays) < AM.MAX_PLAYS:
            if AM._turn(g) == ON.CHANCE:
                g = AM._consume(g, ON.Draw(draws[AM._street(g)]))
                continue
            past, choices = w.info()
            n = PM.nch(choices)
            row = bp.get((past, RM._bucket(AM._street(g), holes[AM._turn(g)], g.board), choices))
            p = row[0][:n].astype(np.float64) if row is not None else np.ones(n)
            e = int(PM.edges(choices)[rng.choice(n, p=p / p.sum())])
            a = o.ora_nlhe_snap(C.byref(g), o.ora_nlhe_actionize(C.byref(g), e, 0))
            a = (a.kind, 0 if a.kind in (ON.FOLD, ON.CHECK) else a.chips, 0)
            plays.append((a[0], a[1]))
            w.push(a)
            g = AM._consume(g, a)
        return AivatHand(holes, draws[: AM._street(g)], plays, seat=int(rng.integers(2)), board_mode=1)

    # ---- the distinct hands, and on the host what the composed route needs: every key a hand asks for
    t0 = time.perf_counter()
    hands = [play() for _ in range(args.distinct)]
    play_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    keys, probes = [], []
    for h in hands:
        rec, trace = AM.Recorder(), []
        assert AM.corrections(h, rec, trace)[0] == AM.OK
        keys.append(list(rec.asked))
        probes.append(sum(ev["deals"] for ev in trace if ev["kind"] == "chance"))
    replay_s = time.perf_counter() - t0
    say(f"{args.distinct} hands played in {play_s:.1f} s and replayed for their keys in {replay_s:.1f} s: "
        f"{np.mean([len(h.plays) for h in hands]):.1f} plays, {np.mean([len(k) for k in keys]):.1f} keys, {np.mean(probes):.1f} chance-deal probes a hand")

    # ---- the table: the rows the hands ask for, and filler
    for ks in keys:
        for k in ks:
            bp.get(k)
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
    say(f"table: 2^{args.cap_log2} slots, {past.size} rows loaded ({len(own)} of them infosets the hands ask for)")

    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    CHUNK = 1 << 21
    buf = (np.zeros((CHUNK, A), ENC_DTYPE), np.zeros(CHUNK, np.uint8), np.zeros(CHUNK, np.uint8))

    def memory(kp, kq, kc, keep=False):
        """rp_nlhe_memory over all keys, CHUNK at a time into one reused buffer; keep: the answers of the first chunk"""
        out = None
        for at in range(0, kp.size, CHUNK):
            m = min(CHUNK, kp.size - at)
            _lib.check(s._lib.rp_nlhe_memory(s._h, m, ptr(kp[at:]), ptr(kq[at:]), ptr(kc[at:]), ptr(buf[0]), ptr(buf[1]), ptr(buf[2])))
            if keep and at == 0:
                out = (buf[0][:m].copy(), buf[2][:m].copy())
        return out

    flat = [k for ks in keys for k in ks]
    first = np.cumsum([0] + [len(ks) for ks in keys])
    dk = (np.array([k[0] for k in flat], np.uint64), np.array([k[1] for k in flat], np.uint32), np.array([k[2] for k in flat], np.uint64))
    assert dk[0].size <= CHUNK
    menc, mfound = memory(*dk, keep=True)
    answered = {k: (menc[i]["weight"].copy(), menc[i]["payoff"].copy()) for i, k in enumerate(flat) if mfound[i]}
    want = [AM.corrections(h, answered) for h in hands]

    out = {"device": torch.cuda.get_device_name(0), "cap_log2": args.cap_log2, "rows_loaded": int(past.size), "distinct_hands": args.distinct,
           "plays_per_hand": float(np.mean([len(h.plays) for h in hands])), "keys_per_hand": float(np.mean([len(k) for k in keys])),
           "chance_deal_probes_per_hand": float(np.mean(probes)), "runs": args.runs,
           "host_replay": {"self_play_seconds": play_s, "keying_seconds_for_the_distinct_hands": replay_s,
                           "how": "the two-game model over the CPU oracle through ctypes; in no timed window below"},
           "timing": "host clock around host-form calls that end in a device synchronise; fused and composed alternate; median / min / max of "
                     "the runs; composed = the rp_nlhe_memory calls alone, a lower bound of that route",
           "results": {}}
    for n in [int(b) for b in args.batches.split(",")]:
        idx = np.arange(n) % args.distinct
        packed = AivatHand.pack(hands)[idx]
        rounds, rest = divmod(n, args.distinct)  # the batch is the distinct hands in order, over and over
        kidx = np.concatenate([np.arange(first[-1])] * rounds + [np.arange(first[rest])])
        kp, kq, kc = (np.ascontiguousarray(d[kidx]) for d in dk)
        got = s.aivat(packed)  # warm-up of both shapes, and the comparison of their answers
        memory(kp, kq, kc)
        same = True
        for j, i in enumerate(idx):
            w = want[i]
            same = same and got["status"][j] == w[0] and (got["n_action"][j], got["n_chance"][j]) == w[5:] and all(
                np.float32(got[f][j]).view(np.uint32) == np.float32(w[1 + k]).view(np.uint32) for k, f in enumerate(("hero", "villain", "chance", "total")))
        tf, tc = [], []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            s.aivat(packed)
            tf.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            memory(kp, kq, kc)
            tc.append(time.perf_counter() - t0)
        n_probes = int(sum(probes[i] for i in idx))
        res = {}
        for name, ts in (("fused", tf), ("composed_lower_bound", tc)):
            med = float(np.median(ts))
            res[name] = {"seconds": ts, "median_s": med, "min_s": min(ts), "max_s": max(ts), "hands_per_s": n / med}
        res["fused"]["chance_deal_probes_per_s"] = n_probes / res["fused"]["median_s"]
        res["bit_identical"] = bool(same)
        res["keys"] = int(kp.size)
        res["bytes_moved"] = {"fused_up": n * 192, "fused_back": n * 19, "composed_up": int(kp.size) * 20, "composed_back": int(kp.size) * 146}
        res["fused_faster_beyond_spread"] = bool(max(tf) < min(tc))
        res["speedup_of_medians"] = res["composed_lower_bound"]["median_s"] / res["fused"]["median_s"]
        out["results"][str(n)] = res
        say(f"batch {n}: fused {res['fused']['median_s'] * 1e3:.2f} ms [{min(tf) * 1e3:.2f}, {max(tf) * 1e3:.2f}], composed >= "
            f"{res['composed_lower_bound']['median_s'] * 1e3:.2f} ms [{min(tc) * 1e3:.2f}, {max(tc) * 1e3:.2f}], same bits: {same}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps({b: {"fused_hands_per_s": r["fused"]["hands_per_s"], "speedup_of_medians": r["speedup_of_medians"],
                          "bit_identical": r["bit_identical"]} for b, r in out["results"].items()}))


if __name__ == "__main__":
    main()

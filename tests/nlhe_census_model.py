"""CPU model of the blueprint census (include/rp_mi355x.h, THE BLUEPRINT CENSUS): rp_nlhe_table_census's record and the four
summaries, following the header's arithmetic contract with explicit loops — numpy's add.reduce is pairwise and is not used for any
fold.  Python floats are IEEE f64; np.float32 scalars round every operation to f32.

tests/test_nlhe_census_model.py pins the model: integers, extremes and lists against a dict-based group-by of the expanded rows,
every float sum against math.fsum within the bound of a left fold."""
import numpy as np

import nlhe_policy_model as PM
from robopoker_amd.nlhe import CENSUS_DTYPE

A, F = PM.A, np.float32
TOP, SEGMENT, STREETS, CODES = 64, 65536, 5, 32
SUMS = ("ratio", "weight", "total", "regret", "payoff")


def expand(slot, past, present, choices, enc):
    """the rows of the SQL table in the contract's order (slot ascending, then action): one dict per (infoset, action a < n_actions)
    with street, code, slot, a, the Encounter's four fields, dec_total (f32), rated and ratio (f32, None where not rated)"""
    out = []
    with np.errstate(all="ignore"):
        for i in np.argsort(np.asarray(slot), kind="stable"):
            n = PM.nch(choices[i])
            dec_total = F(0.0)
            for a in range(n):
                dec_total = F(dec_total + F(enc[i][a]["weight"]))
            rated = bool(dec_total != F(0.0))
            for a in range(n):
                e = enc[i][a]
                w = F(e["weight"])
                out.append(dict(key=(int(past[i]), int(present[i]), int(choices[i])), n_actions=n, slot=int(slot[i]), a=a,
                                street=min(int(present[i]) >> 8, 4), code=(int(choices[i]) >> (5 * a)) & 31, weight=w, regret=F(e["regret"]),
                                payoff=F(e["payoff"]), visits=int(e["visits"]), dec_total=dec_total, rated=rated,
                                ratio=F(w / dec_total) if rated else None))
    return out


def terms_of(row):
    """the f64 terms a row adds to its cell's five sums (None: nothing is added)"""
    return dict(ratio=float(row["ratio"]) if row["rated"] else None, weight=float(row["weight"]), total=float(row["dec_total"]),
                regret=float(row["regret"]), payoff=float(row["payoff"]))


def fold_sums(rows, n_segments, mode="segmented"):
    """{(street, code): {sum name: f64}} of expanded rows (in the contract's order).  "segmented": the contract — a left fold inside
    each segment of 65 536 slots, then a left fold of the segment sums; "global": one left fold in the contract's row order;
    "descending": one left fold over the slots in DESCENDING order (actions still ascending) — the two orders the contract is not."""
    if mode == "descending":
        rows = sorted(rows, key=lambda r: (-r["slot"], r["a"]))
    cells = {}
    for r in rows:
        seg = r["slot"] // SEGMENT if mode == "segmented" else 0
        acc = cells.setdefault((r["street"], r["code"]), {}).setdefault(seg, dict.fromkeys(SUMS, 0.0))
        for k, x in terms_of(r).items():
            if x is not None:
                acc[k] = acc[k] + x
    out = {}
    for cell, segs in cells.items():
        tot = dict.fromkeys(SUMS, 0.0)
        for seg in range(n_segments if mode == "segmented" else 1):
            part = segs.get(seg, dict.fromkeys(SUMS, 0.0))
            for k in SUMS:
                tot[k] = tot[k] + part[k]
        out[cell] = tot
    return out


def census(slot, past, present, choices, enc, epoch=0, slots=256):
    """the rp_census record (a CENSUS_DTYPE scalar array) of a table of `slots` slots holding infoset i at slot[i]"""
    rec = np.zeros((), CENSUS_DTYPE)
    rec["epoch"], rec["slots"] = epoch, slots
    rows = expand(slot, past, present, choices, enc)
    sums = fold_sums(rows, (slots + SEGMENT - 1) // SEGMENT)
    seen, per_info = set(), {}
    for r in rows:
        c = rec["cell"][r["street"]][r["code"]]
        first = c["rows"] == 0
        c["rows"] += 1
        if r["rated"]:
            c["rated"] += 1
            c["dominant"] += 1 if r["ratio"] > F(0.5) else 0
        c["visits"] += r["visits"]
        for f, pick in (("max_regret", max), ("min_regret", min), ("max_weight", max), ("max_payoff", max), ("min_payoff", min),
                        ("max_visits", max), ("min_visits", min)):
            v = r[f[4:]]
            c[f] = v if first else pick(c[f], v)
        if r["key"] not in seen:
            seen.add(r["key"])
            rec["infosets"][r["street"]] += 1
        m = per_info.setdefault(r["key"], dict(n=r["n_actions"], min_visits=r["visits"], max_regret=r["regret"], max_abs=abs(r["regret"])))
        m["min_visits"], m["max_regret"], m["max_abs"] = min(m["min_visits"], r["visits"]), max(m["max_regret"], r["regret"]), max(m["max_abs"], abs(r["regret"]))
    for (s, e), tot in sums.items():
        for k in SUMS:
            rec["cell"][s][e][k] = tot[k]
    cold = sorted(per_info.items(), key=lambda kv: (kv[1]["min_visits"],) + kv[0])[:TOP]
    hot = sorted(per_info.items(), key=lambda kv: (-float(kv[1]["max_abs"]),) + kv[0])[:TOP]
    rec["n_cold"], rec["n_hot"] = len(cold), len(hot)
    for name, lst, field, src in (("cold", cold, "visits", "min_visits"), ("hot", hot, "regret", "max_regret")):
        for i, (key, m) in enumerate(lst):
            x = rec[name][i]
            x["past"], x["present"], x["choices"], x["edges"] = key[0], key[1], key[2], m["n"]
            x[field] = m[src]
    return rec


def _cells(rec, streets):
    """f64 sums over the cells of `streets`, street then code ascending, and the extremes over the non-empty ones"""
    t = dict(rows=0, visits=0, regret=0.0, weight=0.0, payoff=0.0)
    ext = {}
    for s in streets:
        for e in range(CODES):
            c = rec["cell"][s][e]
            for k in ("regret", "weight", "payoff"):
                t[k] = t[k] + float(c[k])
            if c["rows"] == 0:
                continue
            for f, pick in (("max_regret", max), ("min_regret", min), ("max_weight", max), ("max_payoff", max), ("min_payoff", min),
                            ("max_visits", max), ("min_visits", min)):
                ext[f] = c[f] if f not in ext else pick(ext[f], c[f])
            t["rows"] += int(c["rows"])
            t["visits"] += int(c["visits"])
    return t, ext


def stats(rec):
    t, ext = _cells(rec, range(STREETS))
    out = dict(infosets=int(sum(int(x) for x in rec["infosets"])), edges=t["rows"])
    names = ("avg_regret", "max_regret", "min_regret", "avg_weight", "max_weight", "avg_payoff", "max_payoff", "min_payoff", "avg_visits")
    if t["rows"] == 0:
        out.update({k: F(0.0) for k in names}, max_visits=0, min_visits=0)
        return out
    n = float(t["rows"])
    out.update(avg_regret=F(t["regret"] / n), avg_weight=F(t["weight"] / n), avg_payoff=F(t["payoff"] / n), avg_visits=F(float(t["visits"]) / n))
    out.update({k: F(ext[k]) for k in ("max_regret", "min_regret", "max_weight", "max_payoff", "min_payoff")})
    out.update(max_visits=int(ext["max_visits"]), min_visits=int(ext["min_visits"]))
    return out


def street_stats(rec):
    out = []
    for s in range(STREETS):
        t, _ = _cells(rec, [s])
        n = float(t["rows"])
        avg = {k: (F(t[k] / n) if t["rows"] else F(0.0)) for k in ("regret", "weight", "payoff")}
        out.append(dict(street="PFTR?"[s], infosets=int(rec["infosets"][s]), edges=t["rows"], avg_regret=avg["regret"], avg_weight=avg["weight"],
                        avg_payoff=avg["payoff"], avg_visits=F(float(t["visits"]) / n) if t["rows"] else F(0.0)))
    return out


def saturation(rec):
    _, ext = _cells(rec, range(STREETS))
    ext = {k: ext.get(k, 0) for k in ("max_regret", "min_regret", "max_weight", "max_payoff", "min_payoff", "max_visits")}
    precision = np.finfo(np.float32).max
    w, r = F(ext["max_weight"]), F(max(abs(F(ext["max_regret"])), abs(F(ext["min_regret"]))))
    return dict(max_weight=w, max_regret=r, max_payoff=F(max(abs(F(ext["max_payoff"])), abs(F(ext["min_payoff"])))), max_visits=int(ext["max_visits"]),
                precision_f32=precision, weight_pct=F(F(w / precision) * F(100.0)), regret_pct=F(F(r / precision) * F(100.0)))


def grid_usage(rec):
    out = []
    for s in range(STREETS):
        rows = []
        for e in range(CODES):
            c = rec["cell"][s][e]
            if c["rows"] == 0:
                continue
            rated = int(c["rated"])
            rows.append(dict(street=s, code=e, avg_freq=F(float(c["ratio"]) / float(rated)) if rated else F(0.0),
                             weighted_freq=F(float(c["weight"]) / float(c["total"])) if float(c["total"]) != 0.0 else F(0.0),
                             n_decisions_with_edge=int(c["rows"]), n_dominant=int(c["dominant"]), _rated=rated != 0))
        rows.sort(key=lambda g: (not g["_rated"], -float(g["avg_freq"]), g["code"]))
        out += rows
    for g in out:
        del g["_rated"]
    return out

"""Pins tests/nlhe_census_model.py, the CPU model the device census is compared with bit for bit (tests/test_gpu_nlhe_census.py),
independently of the model's own loops:
  * integer fields (rated and dominant included, from a float32 fold and division of the group-by's own), extremes and the ranked
    lists against a dict-based group-by straight from the arrays;
  * every float sum against math.fsum of the same terms within the bound of a recursive sum of n terms,
    |fold - exact| <= gamma(n - 1) * sum|x| with gamma(m) = m u / (1 - m u), u = 2^-53 (Higham, Accuracy and Stability, §4.2).
    The segmented fold stays inside it: every fold's first addition is to +0.0 and exact, so is the addition of an empty segment's
    +0.0, and s non-empty segments of n_1 + .. + n_s = n terms round (n_1 - 1) + .. + (n_s - 1) + (s - 1) = n - 1 additions;
  * the two-segment fixture can tell the contract's order from the two natural others."""
import math
import struct

import numpy as np
import pytest

import nlhe_census_cases as K
import nlhe_census_model as CM

U = 2.0 ** -53


def gamma(m):
    return m * U / (1 - m * U)


def bits64(x):
    return struct.pack("<d", float(x))


@pytest.fixture(scope="module")
def corner():
    return K.corner_table()


@pytest.fixture(scope="module")
def two_segments():
    return K.random_table(17, 3000, seed=5, tie_every=7)


def group_by(t):
    """{(street, code): rows} and {key: rows} straight from the arrays, without the model's expansion; a row is (weight, regret,
    payoff, visits, ratio): ratio = weight / the infoset's float32 left fold of its weights, None where that total is zero"""
    cells, infos = {}, {}
    for i in range(t.keys[0].size):
        past, present, choices = (int(k[i]) for k in t.keys)
        n = 0
        while n < 9 and (choices >> (5 * n)) & 31:
            n += 1
        total = np.float32(0.0)
        for w in t.enc[i]["weight"][:n]:
            total = np.float32(total + w)
        a = 0
        while a < 9 and (choices >> (5 * a)) & 31:
            with np.errstate(all="ignore"):
                ratio = None if total == 0 else np.float32(t.enc[i][a]["weight"] / total)
            row = (float(t.enc[i][a]["weight"]), float(t.enc[i][a]["regret"]), float(t.enc[i][a]["payoff"]), int(t.enc[i][a]["visits"]), ratio)
            cells.setdefault((min(present >> 8, 4), (choices >> (5 * a)) & 31), []).append(row)
            infos.setdefault((past, present, choices), []).append(row)
            a += 1
    return cells, infos


@pytest.mark.parametrize("name", ["corner", "two_segments"])
def test_integers_extremes_and_lists_against_a_group_by(name, request):
    t = request.getfixturevalue(name)
    rec = t.model(CM)
    cells, infos = group_by(t)
    assert rec["epoch"] == t.epoch and rec["slots"] == t.slots
    for s in range(5):
        assert rec["infosets"][s] == sum(1 for k in infos if min(k[1] >> 8, 4) == s)
        for e in range(32):
            c, rows = rec["cell"][s][e], cells.get((s, e), [])
            assert c["rows"] == len(rows) and c["visits"] == sum(r[3] for r in rows) and c["reserved"] == 0
            assert c["rated"] == sum(1 for r in rows if r[4] is not None)
            assert c["dominant"] == sum(1 for r in rows if r[4] is not None and r[4] > np.float32(0.5))
            if not rows:
                assert c.tobytes() == bytes(104)
                continue
            assert c["max_weight"] == max(r[0] for r in rows)
            assert c["max_regret"] == max(r[1] for r in rows) and c["min_regret"] == min(r[1] for r in rows)
            assert c["max_payoff"] == max(r[2] for r in rows) and c["min_payoff"] == min(r[2] for r in rows)
            assert c["max_visits"] == max(r[3] for r in rows) and c["min_visits"] == min(r[3] for r in rows)
    assert rec["cell"][:, 0]["rows"].sum() == 0  # code 0 is no edge
    cold = sorted(infos, key=lambda k: (min(r[3] for r in infos[k]),) + k)[:64]
    hot = sorted(infos, key=lambda k: (-max(abs(r[1]) for r in infos[k]),) + k)[:64]
    assert rec["n_cold"] == len(cold) == rec["n_hot"] == len(hot) == min(64, len(infos))
    for i, k in enumerate(cold):
        x = rec["cold"][i]
        assert (int(x["past"]), int(x["present"]), int(x["choices"])) == k and x["edges"] == len(infos[k])
        assert x["visits"] == min(r[3] for r in infos[k]) and x["regret"] == 0
    for i, k in enumerate(hot):
        x = rec["hot"][i]
        assert (int(x["past"]), int(x["present"]), int(x["choices"])) == k and x["edges"] == len(infos[k])
        assert x["regret"] == max(r[1] for r in infos[k]) and x["visits"] == 0
    assert rec["cold"][len(cold):].tobytes() == bytes(32 * (64 - len(cold))) and rec["hot"][len(hot):].tobytes() == bytes(32 * (64 - len(hot)))


@pytest.mark.parametrize("name", ["corner", "two_segments"])
def test_float_sums_against_fsum(name, request):
    t = request.getfixturevalue(name)
    rec = t.model(CM)
    terms = {}
    for r in CM.expand(t.slot, *t.keys, t.enc):
        for k, x in CM.terms_of(r).items():
            if x is not None:
                terms.setdefault((r["street"], r["code"], k), []).append(x)
    checked = 0
    for (s, e, k), xs in terms.items():
        got, exact = float(rec["cell"][s][e][k]), math.fsum(xs)
        assert abs(got - exact) <= gamma(len(xs) - 1) * math.fsum(abs(x) for x in xs), (s, e, k)
        checked += 1
    assert checked > 100


def test_the_corner_table_holds_its_corners(corner):
    rec = corner.model(CM)
    assert corner.keys[0].size == 150 and K.wraps(corner)
    assert all(rec["infosets"][s] > 0 for s in range(5))
    assert rec["cell"][3][31]["rows"] > 0 and rec["cell"][2][12]["rows"] >= 3       # codes up to 31; one code three times in an infoset
    assert (rec["cell"]["rows"] > rec["cell"]["rated"]).any()                        # rows of a decision without weight
    assert rec["cell"][0][3]["dominant"] >= 1 and rec["cell"][0][3]["rated"] >= 2    # 0.5f is not dominant, its successor is
    r = [x for x in CM.expand(corner.slot, *corner.keys, corner.enc) if x["key"][0] in (7, 8) and x["a"] == 0]
    assert sorted(float(x["ratio"]) for x in r) == [0.5, 0.5 + 2.0 ** -24]
    assert rec["cold"][0]["visits"] == 0 and rec["cold"][63]["visits"] > 0
    top = [x for x in rec["hot"][:3]]
    assert sorted(float(x["regret"]) for x in top) == [-3.0, 5.0, float(np.float32(1e30))]  # MAX(regret) is what is reported
    assert [int(x["past"]) for x in top] == sorted(int(x["past"]) for x in top)            # the key settles the tie


def test_the_two_segment_fixture_tells_the_orders_apart(two_segments):
    t = two_segments
    assert (t.slot < CM.SEGMENT).sum() > 1000 and (t.slot >= CM.SEGMENT).sum() > 1000
    rows = CM.expand(t.slot, *t.keys, t.enc)
    seg, glob, desc = (CM.fold_sums(rows, 2, mode) for mode in ("segmented", "global", "descending"))
    apart = [(cell, k) for cell in seg for k in CM.SUMS
             if bits64(seg[cell][k]) != bits64(glob[cell][k]) and bits64(seg[cell][k]) != bits64(desc[cell][k])]
    assert apart, "no cell's segmented fold differs in bits from both the global fold and the descending one"
    rec = t.model(CM)
    (s, e), k = apart[0]
    assert bits64(rec["cell"][s][e][k]) == bits64(seg[(s, e)][k])


def test_summaries_of_the_model_are_consistent(corner):
    rec = corner.model(CM)
    st, per, sat, grid = CM.stats(rec), CM.street_stats(rec), CM.saturation(rec), CM.grid_usage(rec)
    assert st["infosets"] == 150 and st["edges"] == int(rec["cell"]["rows"].sum()) == sum(p["edges"] for p in per)
    assert [p["street"] for p in per] == list("PFTR?") and sum(p["infosets"] for p in per) == 150
    assert sat["max_visits"] == 0xFFFFFFFF == st["max_visits"] and sat["max_regret"] == np.float32(1e30)
    assert len(grid) == int((rec["cell"]["rows"] > 0).sum())
    for a, b in zip(grid, grid[1:]):
        assert a["street"] <= b["street"]

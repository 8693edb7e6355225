"""The blueprint census on the device (rp_nlhe_table_census and its _device form) against tests/nlhe_census_model.py, which
tests/test_nlhe_census_model.py pins on the CPU.  Every comparison is on bytes — counts, the exact sum of visits, the five f64 sums
of every cell, the lists — except the extremes, which the contract compares as values (the sign of a zero extreme is unspecified).

What the scan must get right: which slots are ready (keys off their home slot, a chain that wraps past the last slot, a full and an
empty table), the float order (slot order inside a segment of 65 536 slots, then segment order: two and four segments), rows beyond an
infoset's actions, two actions of one infoset in one cell, the ranked lists' total orders, and that nothing is written."""
import ctypes as C

import numpy as np
import pytest
import torch

import nlhe_census_cases as K
import nlhe_census_model as CM
from robopoker_amd import _lib
from robopoker_amd.nlhe import CENSUS_DTYPE, NlheSolver, census_cold, census_grid_usage, census_hot, census_stats

pytestmark = pytest.mark.gpu

EXTREMES = ("max_regret", "min_regret", "max_weight", "max_payoff", "min_payoff")


def unsigned_zero_extremes(rec):
    rec = rec.copy()
    for f in EXTREMES:
        rec["cell"][f] = rec["cell"][f] + np.float32(0.0)  # -0.0 + 0.0 = +0.0; everything else is unchanged
    return rec


def assert_same(got, want, what=""):
    for f in EXTREMES:
        assert np.array_equal(got["cell"][f], want["cell"][f]), (what, f)
    a, b = unsigned_zero_extremes(got), unsigned_zero_extremes(want)
    if a.tobytes() != b.tobytes():  # name the field before failing
        for f in CENSUS_DTYPE.names:
            if f == "cell":
                for g in a["cell"].dtype.names:
                    assert a["cell"][g].tobytes() == b["cell"][g].tobytes(), (what, "cell", g, np.argwhere(a["cell"][g] != b["cell"][g])[:4].tolist())
            assert a[f].tobytes() == b[f].tobytes(), (what, f)
    assert a.tobytes() == b.tobytes(), what


def solver_of(t):
    s = NlheSolver(cap_log2=t.cap_log2, batch=1, seed=1)
    if t.keys[0].size:
        s.load(*t.keys, t.enc, epoch=t.epoch)
    return s


def device_form(s):
    out = s.table_census_device()
    s.sync()
    return out.cpu().numpy().view(CENSUS_DTYPE)[0]


def test_the_corner_table(gpu):
    t = K.corner_table()
    assert t.keys[0].size == 150 and K.wraps(t)
    s, want = solver_of(t), t.model(CM)
    got = s.table_census()
    assert_same(got, want, "corner")
    assert got["epoch"] == 3 and got["slots"] == 256 and int(got["infosets"].sum()) == 150 == s.counters()[2]
    assert got["cell"][2][12]["rows"] >= 3 and got["cell"][3][31]["rows"] > 0 and (got["cell"]["rows"] > got["cell"]["rated"]).any()
    assert [float(x["max_regret"]) for x in census_hot(got, 3)] == [5.0, float(np.float32(1e30)), -3.0]
    # the three forms answer the same bytes, and a repeated call too
    assert device_form(s).tobytes() == got.tobytes() == s.table_census().tobytes()
    assert census_stats(got)["max_visits"] == 0xFFFFFFFF and len(census_grid_usage(got)) == int((want["cell"]["rows"] > 0).sum())


def test_a_full_and_an_empty_table(gpu):
    full = K.random_table(8, 256, seed=2)
    assert sorted(full.slot) == list(range(256))
    s = solver_of(full)
    got = s.table_census()
    assert_same(got, full.model(CM), "full")
    assert got["n_cold"] == got["n_hot"] == 64 and int(got["infosets"].sum()) == 256
    e = NlheSolver(cap_log2=8, batch=1, seed=1)
    want = np.zeros((), CENSUS_DTYPE)
    want["slots"] = 256
    for got in (e.table_census(), device_form(e)):
        assert got.tobytes() == want.tobytes()
    assert census_cold(got) == [] and census_stats(got)["edges"] == 0


@pytest.mark.parametrize("n", [10, 64, 65])
def test_ranked_lists_and_their_ties(gpu, n):
    t = K.list_table(n)
    got, want = solver_of(t).table_census(), t.model(CM)
    assert_same(got, want, n)
    assert got["n_cold"] == got["n_hot"] == min(n, 64)
    cold, hot = census_cold(got), census_hot(got)
    if n >= 64:  # values repeat: the key decides, ascending
        assert len({c["visits"] for c in cold}) < len(cold) and len({abs(float(h["max_regret"])) for h in hot}) < len(hot)
        for lst, val in ((cold, lambda c: c["visits"]), (hot, lambda h: -max(abs(float(r)) for r in t.enc["regret"][t.keys[0] == np.uint64(h["past"])][0][: h["edges"]]))):
            ranks = [(val(x), x["past"], x["present"], x["choices"]) for x in lst]
            assert ranks == sorted(ranks)


def test_visit_counts_that_would_be_nans_as_floats(gpu):
    t = K.nan_visits_table()
    got, want = solver_of(t).table_census(), t.model(CM)
    assert_same(got, want, "nan patterns")
    assert got["n_cold"] == 12 and {c["visits"] for c in census_cold(got)} <= set(K.NAN_PATTERNS)
    assert [c["visits"] for c in census_cold(got)] == sorted(c["visits"] for c in census_cold(got))


@pytest.mark.parametrize("cap_log2,n,seed", [(17, 3000, 5), (18, 4000, 6)])
def test_segments_fold_in_order(gpu, cap_log2, n, seed):
    t = K.random_table(cap_log2, n, seed=seed, tie_every=7)
    segs = np.bincount(t.slot // CM.SEGMENT, minlength=t.slots // CM.SEGMENT)
    assert segs.size == (2 if cap_log2 == 17 else 4) and (segs > 500).all()
    s, want = solver_of(t), t.model(CM)
    got = s.table_census()
    assert_same(got, want, cap_log2)
    assert device_form(s).tobytes() == got.tobytes()
    # a fold in another order would have been seen: some cell's sum differs in bits between the contract's order and a plain fold
    rows = CM.expand(t.slot, *t.keys, t.enc)
    plain = CM.fold_sums(rows, 1, "global")
    assert any(np.float64(plain[(se)][k]).tobytes() != want["cell"][se[0]][se[1]][k].tobytes() for se in plain for k in CM.SUMS)


def test_a_trained_table(gpu):
    s = NlheSolver(cap_log2=12, batch=2, seed=2)
    for _ in range(3):
        s.step()
    past, present, choices, enc = s.export()  # in slot order: one segment, so the order is all the model needs
    got = s.table_census()
    assert_same(got, CM.census(np.arange(past.size), past, present, choices, enc, epoch=s.epoch, slots=1 << 12), "trained")
    assert int(got["infosets"].sum()) == s.counters()[2] == past.size > 100 and got["epoch"] == s.epoch == 3
    assert got["infosets"][4] == 0 and census_stats(got)["edges"] == int(CM.PM.nch_rows(choices).sum())


def test_nothing_is_written_and_steps_are_not_disturbed(gpu):
    def table(s):
        return tuple(x.tobytes() for x in s.export()) + (s.epoch, s.counters())

    def by_key(s):
        """the table as a key -> Encounters map: which slot a key takes depends on the order in which concurrent trees insert"""
        past, present, choices, enc = s.export()
        order = np.lexsort((choices, present, past))
        return tuple(x[order].tobytes() for x in (past, present, choices, enc)) + (s.epoch, s.counters())

    a, b = (NlheSolver(cap_log2=12, batch=2, seed=4) for _ in range(2))
    a.step(), b.step()
    before = table(a)
    first = a.table_census()
    assert table(a) == before and a.table_census().tobytes() == first.tobytes()
    out = a.table_census_device()  # queued between two steps, not waited for
    a.step(), b.step()
    a.sync()
    assert out.cpu().numpy().view(CENSUS_DTYPE)[0].tobytes() == first.tobytes()
    assert by_key(a) == by_key(b)


def test_an_import_that_names_a_key_twice_keeps_the_last_rows(gpu):
    """rp_nlhe_import uploads its rows by one scatter launch per chunk: a key given twice in one call still ends with its LAST Encounters"""
    t = K.list_table(40)
    twice = tuple(np.concatenate([k, k[:25][::-1]]) for k in t.keys)
    later = t.enc[:25][::-1].copy()
    later["visits"] += 100
    s = NlheSolver(cap_log2=8, batch=1, seed=1)
    s.load(*twice, np.concatenate([t.enc, later]), epoch=3)
    want = t.enc.copy()
    want["visits"][:25] += 100
    want = K.garbage_beyond(want, t.keys[2])
    assert s.counters()[2] == 40
    assert_same(s.table_census(), CM.census(t.slot, *t.keys, want, epoch=3, slots=256), "named twice")


def test_null_arguments_leave_the_handle_usable(gpu):
    lib = _lib.load()
    s = NlheSolver(cap_log2=8, batch=1, seed=1)
    for fn in (lib.rp_nlhe_table_census, lib.rp_nlhe_table_census_device):
        assert fn(s._h, None) == _lib.RP_ERR_INVALID and b"rp_nlhe_table_census" in lib.rp_last_error()
    assert s.table_census()["slots"] == 256

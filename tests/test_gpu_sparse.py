"""Sparse profile (rp_profile_*) on the GPU vs the CPU oracle (ora_profile_*): bit-exact tables and summary entries."""
import numpy as np
import pytest
import torch

import oracle
from robopoker_amd import _lib
from robopoker_amd.sparse import DeviceBatch, SparseProfile, synthetic_batch

pytestmark = pytest.mark.gpu
FIELDS = ("weight", "regret", "payoff", "visits")


def same(a, b):
    for f in FIELDS:
        if a[f].dtype.kind == "f":  # equal bits would also be equal NaNs: a table never holds one
            assert not np.isnan(a[f]).any(), f"{f}: NaN in the table"
        assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), f"{f}: {np.count_nonzero(a[f].view(np.uint32) != b[f].view(np.uint32))} cells differ"


@pytest.mark.parametrize("regret,weight", [("linear", "linear"), ("floored", "linear"), ("summed", "constant"),
                                           ("discounted", "quadratic"), ("asymmetric", "exponential")])
def test_ordered_apply_bit_exact(gpu, regret, weight):
    n_rows, A = 500, 9  # few rows: the popular ones collect thousands of touches per batch
    dr = np.array([100, 10, 0, 50, 0, 0, 0, 0, 0], dtype=np.float32)  # NLHE-style bias (kicker/src/edge.rs:61-72)
    g = SparseProfile(n_rows, A, regret, weight, default_regret=dr)
    o = oracle.OracleProfile(n_rows, A, regret, weight, default_regret=dr)
    for e in range(5):
        batch = synthetic_batch(20000, n_rows, A, seed=100 + e)
        g.apply(DeviceBatch(*batch), "ordered")
        o.apply(batch)
    g.sync()
    assert g.epoch() == o.epoch() == 5
    same(g.rows(np.arange(n_rows)), o.rows(np.arange(n_rows)))


@pytest.mark.parametrize("regret,weight,A", [("linear", "linear", 9), ("floored", "quadratic", 16), ("summed", "exponential", 2)])
def test_composed_apply_and_entries_bit_exact(gpu, regret, weight, A):
    n_rows = 300
    g = SparseProfile(n_rows, A, regret, weight)
    o = oracle.OracleProfile(n_rows, A, regret, weight)
    assert g.entry_bytes() == o.entry_bytes() == 16 + 32 * A
    for e in range(4):
        batch = synthetic_batch(15000, n_rows, A, seed=7 + e)
        db = DeviceBatch(*batch)
        # entries first (same epoch), then the local composed apply
        buf = torch.zeros(db.n * g.entry_bytes(), dtype=torch.uint8, device="cuda")
        n = g.summarize(db, buf.data_ptr())
        exp = o.summarize(batch)
        assert n * g.entry_bytes() == exp.size
        assert np.array_equal(buf[: exp.size].cpu().numpy(), exp), "summary entries differ"
        g.apply(db, "composed")
        o.fold(exp)
    g.sync()
    assert g.epoch() == o.epoch() == 4
    same(g.rows(np.arange(n_rows)), o.rows(np.arange(n_rows)))


@pytest.mark.parametrize("n_rows,A,n", [(50000, 9, 70000), (300, 9, 66000), (1 << 16, 16, 131073)])
def test_batches_just_past_one_scan_tile_set_bit_exact(gpu, n_rows, A, n):
    # more than ss::SCAN_ONE = 65 536 Decisions: the run lengths and the rows -> blocks index come from the TILED scans (tile sums,
    # scan of the sums, tiles), few rows / many rows / the widest rows
    g = SparseProfile(n_rows, A, "linear", "linear")
    o = oracle.OracleProfile(n_rows, A, "linear", "linear")
    for e in range(2):
        batch = synthetic_batch(n, n_rows, A, seed=n + e)
        db = DeviceBatch(*batch)
        buf = torch.zeros(db.n * g.entry_bytes(), dtype=torch.uint8, device="cuda")
        k = g.summarize(db, buf.data_ptr())
        exp = o.summarize(batch)
        assert k * g.entry_bytes() == exp.size and np.array_equal(buf[: exp.size].cpu().numpy(), exp), "summary entries differ"
        g.apply(db, "composed")
        o.fold(exp)
    g.sync()
    rows = np.unique(batch[0])[:5000]
    same(g.rows(rows), o.rows(rows))


@pytest.mark.parametrize("n_rows,A", [(1 << 19, 2), (300, 9), (1 << 10, 9), (3, 9)])  # 3 rows: more than 64 x 64 touches of one row, folded in k_seg_fold
def test_small_batches_prepared_by_one_workgroup_bit_exact(gpu, n_rows, A):
    # at most ss::SORT_ONE = 16 384 Decisions (the reference's 128 trees emit ~10^4): sort, run lengths and block index in one launch of
    # one workgroup (k_prep_one): one / two / three radix passes (9, 10 and 19 key bits), the sizes around its round and chunk edges,
    # and the first size that goes back to the tiled sort
    g = SparseProfile(n_rows, A, "linear", "linear")
    o = oracle.OracleProfile(n_rows, A, "linear", "linear")
    seen = []
    for e, n in enumerate([1, 63, 64, 65, 1023, 1024, 1025, 9000, 16383, 16384, 16385]):
        batch = synthetic_batch(n, n_rows, A, seed=900 + e)
        g.apply(DeviceBatch(*batch), "composed")
        o.fold(o.summarize(batch))
        seen.append(batch[0])
    g.sync()
    rows = np.unique(np.concatenate(seen))
    same(g.rows(rows), o.rows(rows))


def test_hot_rows_fold_their_block_groups_in_parallel_bit_exact(gpu):
    # 40 rows, 60 000 touches: the popular rows collect > RP_FOLD_GROUP * RP_SPARSE_BLOCK touches (k_hot_fold)
    n_rows, A = 40, 9
    g = SparseProfile(n_rows, A, "linear", "linear")
    o = oracle.OracleProfile(n_rows, A, "linear", "linear")
    for e in range(3):
        batch = synthetic_batch(60000, n_rows, A, seed=50 + e)
        assert np.bincount(batch[0]).max() > 64 * 64 * 2
        db = DeviceBatch(*batch)
        buf = torch.zeros(db.n * g.entry_bytes(), dtype=torch.uint8, device="cuda")
        n = g.summarize(db, buf.data_ptr())
        exp = o.summarize(batch)
        assert np.array_equal(buf[: n * g.entry_bytes()].cpu().numpy(), exp), "summary entries differ"
        g.apply(db, "composed")
        o.fold(exp)
    g.sync()
    same(g.rows(np.arange(n_rows)), o.rows(np.arange(n_rows)))


def test_fold_of_several_ranks_in_rank_order_bit_exact(gpu):
    n_rows, A, world = 400, 7, 3
    g = SparseProfile(n_rows, A, "linear", "linear")
    o = oracle.OracleProfile(n_rows, A, "linear", "linear")
    for e in range(3):
        blobs = []
        for r in range(world):
            batch = synthetic_batch(6000, n_rows, A, seed=1000 * e + r)
            blobs.append(o.summarize(batch))
            db = DeviceBatch(*batch)
            buf = torch.zeros(db.n * g.entry_bytes(), dtype=torch.uint8, device="cuda")
            n = g.summarize(db, buf.data_ptr())
            assert np.array_equal(buf[: n * g.entry_bytes()].cpu().numpy(), blobs[-1])
        allb = np.concatenate(blobs)
        dev = torch.from_numpy(allb).cuda()
        g.fold(dev.data_ptr(), allb.size // g.entry_bytes())
        o.fold(allb)
    g.sync()
    assert g.epoch() == o.epoch() == 3
    same(g.rows(np.arange(n_rows)), o.rows(np.arange(n_rows)))


def test_edges_empty_batch_single_row_and_large_table(gpu):
    g = SparseProfile(1 << 22, 4, "floored", "linear")  # 4M rows x 64 B
    o = oracle.OracleProfile(1 << 22, 4, "floored", "linear")
    empty = tuple(x[:0] for x in synthetic_batch(8, 1 << 22, 4))
    g.apply(DeviceBatch(*empty), "ordered")
    o.apply(empty)
    one = synthetic_batch(3000, 1 << 22, 4, seed=5)
    one = (np.full_like(one[0], 4194303),) + (np.full_like(one[1], 3),) + one[2:]
    one = (one[0], one[1], (one[2] & 7).astype(np.uint16) | 1, one[3], one[4], one[5])
    g.apply(DeviceBatch(*one), "ordered")
    o.apply(one)
    wide = synthetic_batch(50000, 1 << 22, 4, seed=6)
    g.apply(DeviceBatch(*wide), "composed")
    o.fold(o.summarize(wide))
    g.sync()
    rows = np.unique(np.concatenate([wide[0], [4194303, 0, 17]]))
    same(g.rows(rows), o.rows(rows))
    assert g.epoch() == o.epoch() == 3


def test_composed_rejects_sign_dependent_discount_and_bad_arguments(gpu):
    g = SparseProfile(64, 4, "discounted", "linear")
    with pytest.raises(_lib.RpError) as e:
        g.apply(DeviceBatch(*synthetic_batch(10, 64, 4)), "composed")
    assert e.value.code == _lib.RP_ERR_UNSUPPORTED
    with pytest.raises(_lib.RpError):
        SparseProfile(64, 17)
    with pytest.raises(_lib.RpError):
        g.rows([64])


def test_profile_switch_keeps_the_totals_until_it_is_turned_on_again(gpu):
    # rp_profile_profile resets the clocks on an off -> on transition only: after profile(False) the totals of the profiled batches
    # are still readable (the benchmark reads them there)
    g = SparseProfile(64, 4, "linear", "linear")
    g.profile(True)
    g.apply(DeviceBatch(*synthetic_batch(256, 64, 4, seed=3)), "ordered")
    g.profile(False)
    assert g.kernel_time("sort")[1] == 1 and g.kernel_time("apply")[1] == 1
    assert g.kernel_time("sort")[0] >= 0.0
    g.profile(True)
    assert g.kernel_time("sort")[1] == 0 and g.kernel_time("apply")[1] == 0
    with pytest.raises(_lib.RpError) as e:
        g.kernel_time("no_such_kernel")
    assert e.value.code == _lib.RP_ERR_INVALID


def test_full_size_table_properties(gpu):
    # BASELINE configs[3] scale: 2^27 rows x 9 actions (19.3 GB in HBM), one 192 000-Decision Zipf batch per mode.
    # Size-independent properties: visits count the touches exactly, untouched rows keep the default Encounter,
    # ordered and composed agree within the stated tolerance.
    n_rows, A, n = 1 << 27, 9, 192000
    dr = np.array([100, 10, 0, 50, 0, 0, 0, 0, 0], dtype=np.float32)
    batch = synthetic_batch(n, n_rows, A, seed=4)
    db = DeviceBatch(*batch)
    touched, counts = np.unique(batch[0], return_counts=True)
    results = {}
    for mode in ("ordered", "composed"):
        g = SparseProfile(n_rows, A, "linear", "linear", default_regret=dr, max_batch=n)
        g.set_epoch(7)
        g.apply(db, mode)
        g.sync()
        rows = g.rows(touched)
        nact = batch[1][np.searchsorted(np.sort(batch[0]), touched)]  # any touch of the row: |choices| is per row
        order = np.argsort(batch[0], kind="stable")
        nact = batch[1][order][np.concatenate([[0], np.cumsum(counts)[:-1]])]
        for i in (0, len(touched) // 2, len(touched) - 1, int(np.argmax(counts))):
            assert np.all(rows["visits"][i, : nact[i]] == counts[i])
            assert np.all(rows["visits"][i, nact[i]:] == 0)
        assert int(rows["visits"][:, 0].sum()) == n
        probe = np.setdiff1d(np.array([0, 1, 12345678, n_rows - 1], dtype=np.uint32), touched)
        if probe.size:
            un = g.rows(probe)
            assert np.all(un["visits"] == 0) and np.all(un["weight"] == 0) and np.all(un["payoff"] == 0)
            assert np.array_equal(un["regret"], np.tile(dr, (probe.size, 1)))
        assert g.epoch() == 8
        results[mode] = rows
        g.close()
    for f in ("regret", "weight", "payoff"):
        assert np.allclose(results["ordered"][f], results["composed"][f], rtol=2e-4, atol=1e-2), f


@pytest.mark.parametrize("n,bits,kind", [(1, 27, "uniform"), (255, 8, "uniform"), (2049, 27, "uniform"), (70_001, 27, "hot"),
                                         (200_000, 32, "uniform"), (1_500_000, 27, "hot"), (3_000_000, 13, "uniform"),
                                         (50_000, 0, "zero")])
def test_device_sort_scan_and_run_lengths_equal_numpy(gpu, n, bits, kind):
    # csrc/sortscan.hpp (the library's own radix sort / scan / run-length encoding under rp_profile_* and the isomorphism
    # enumeration): the sort must be STABLE (the ordered update applies a row's touches in batch order); sizes around the tile
    # boundaries, past the single-workgroup scan, a multi-level scan (256 x 1465 tile histograms), hot rows (a third of the
    # batch on three keys, like the root infosets of a batch of NLHE trees), bits = 0
    import ctypes as C

    from robopoker_amd import _lib

    rng = np.random.default_rng(n + bits)
    hi = (1 << bits) if bits else 1
    keys = rng.integers(0, hi, size=n, dtype=np.uint64).astype(np.uint32)
    if kind == "hot":
        hot = rng.random(n) < 0.35
        keys[hot] = rng.integers(0, 3, size=int(hot.sum()), dtype=np.uint64).astype(np.uint32) * 1000 + 5
    out = {k: np.zeros(max(n, 1), np.uint32) for k in ("keys", "perm", "uniq", "starts", "counts")}
    n_runs = C.c_uint32()
    scan = np.zeros(max(n, 1), np.uint64)
    p = lambda a: a.ctypes.data  # noqa: E731
    _lib.check(_lib.load().rp_sortscan_selftest(0, n, bits, p(keys), p(out["keys"]), p(out["perm"]), p(out["uniq"]), p(out["starts"]),
                                                p(out["counts"]), C.addressof(n_runs), p(scan)))
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(out["perm"][:n], order.astype(np.uint32)) and np.array_equal(out["keys"][:n], keys[order])
    uniq, starts, counts = np.unique(keys[order], return_index=True, return_counts=True)
    r = n_runs.value
    assert r == len(uniq)
    assert np.array_equal(out["uniq"][:r], uniq) and np.array_equal(out["starts"][:r], starts.astype(np.uint32))
    assert np.array_equal(out["counts"][:r], counts.astype(np.uint32))
    assert np.array_equal(scan[:n], np.concatenate([[0], np.cumsum(keys.astype(np.uint64))[:-1]]).astype(np.uint64))

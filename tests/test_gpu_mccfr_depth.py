"""rp_mccfr_set_frontiers / rp_mccfr_depth_solve on the device (include/rp_mi355x.h, robopoker_amd/csrc/mccfr_subgame.hpp, FR = true):
bit-exact parity with tests/mccfr_depth_model.py (results and rows) at the smallest shapes that can go wrong, the known answer of the
continuation game, the invariances (device against device), the statuses and the refusals that need a handle."""
import os

import numpy as np
import pytest
import torch  # before the library's first HIP call: one HIP runtime per process

import game_tables
import mccfr_depth_cases as C
import mccfr_depth_model as D
import mccfr_subgame_cases as K
import mccfr_subgame_model as M
from robopoker_amd import Game, _lib, games
from robopoker_amd.mccfr import SUBGAME_ENTRY_DTYPE, Solver

pytestmark = pytest.mark.gpu
ROWS_CAP = 24
SEED, FIRST_ID = 11, 5
NONE, ENTRY = _lib.RP_MCCFR_ORIGIN_NONE, _lib.RP_MCCFR_ORIGIN_ENTRY


class Bench:
    """one game, one blueprint: the solver, the model's view of both and the cases; frontier tables are set per test"""

    def __init__(self, name, blueprint):
        self.game = game_tables.game(name) if name == "chance16_mid" else Game(name)
        self.solver = Solver(self.game, "floored", "linear", "external", batch=1, seed=3)
        self.table = M.Table(self.game.table)
        if blueprint == "trained":
            self.solver.solve(1 << 12)
        elif blueprint == "imported":
            self.solver.load_rows(K.corner_rows(self.table), (1 << 24) + 3)
        self.bp = M.Blueprint(self.table, self.solver.export())
        if name == "chance16_mid":
            self.cases = C.chance16_cases(self.table, self.bp)
        elif name.startswith("leduc"):
            self.cases = C.leduc_cases(self.game, self.table, self.bp)
        else:
            self.cases = K.builtin_cases(self.game, self.table, self.bp)
        self.entries = C.stack(self.cases)
        self.labels = [label for label, _ in self.cases]

    def frontiers(self, leaves):
        fr = C.chance16_frontiers(self.game, self.table, leaves) if isinstance(self.game, game_tables.TableGame) else C.builtin_frontiers(self.game, leaves)
        C.set_frontiers(self.solver, fr)
        return fr


_benches = {}


def bench(name, blueprint):
    if (name, blueprint) not in _benches:
        _benches[name, blueprint] = Bench(name, blueprint)
    return _benches[name, blueprint]


def check_against_model(b, fr, entries, origin, iterations, labels=None, rows_cap=ROWS_CAP):
    results, rows = b.solver.depth_solve(entries, origin, iterations=iterations, seed=SEED, first_id=FIRST_ID, rows_cap=rows_cap)
    for i, e in enumerate(entries):
        o = ENTRY if origin is None else (origin if np.isscalar(origin) else origin[i])
        want = D.solve(b.table, b.bp, fr, e, o, index=i, iterations=iterations, seed=SEED, first_id=FIRST_ID)
        try:
            D.compare(results[i], rows[i], want, rows_cap)
        except AssertionError as err:
            raise AssertionError(f"solve {i} ({labels[i] if labels else ''}), origin {o}, {iterations} iterations: {err}") from err
    return results, rows


@pytest.mark.parametrize("iterations", C.ITERATIONS)
@pytest.mark.parametrize("leaves", C.LEAVES)
@pytest.mark.parametrize("name,blueprint", [("leduc", "trained"), ("leduc", "imported"), ("leduc_wide", "trained"), ("leduc_wide", "imported")])
def test_leduc_origin_0_equals_the_model(gpu, name, blueprint, leaves, iterations):
    """root / after check / after raise / check-raise / the board deal observed, both externals, W = 1, 2, 4"""
    b = bench(name, blueprint)
    fr = b.frontiers(leaves)
    results, rows = check_against_model(b, fr, b.entries, 0, iterations, b.labels)
    assert not results["status"].any()
    if iterations == 64:  # the cases do what they are there for
        assert (results["frontiers"] > 0).all() and (rows["kind"] == 1).any()
        observed = [i for i, l in enumerate(b.labels) if "frontier entry" in l]
        assert len(observed) == 6 and all(results["n_actions"][i] == 0 and results["n_rows"][i] > 0 and results["frontiers"][i] == 64 for i in observed)
        assert all((rows[i]["kind"][:results["n_rows"][i]] == 1).all() and (rows[i]["n_actions"][:results["n_rows"][i]] == leaves).all() for i in observed)


@pytest.mark.parametrize("iterations", C.ITERATIONS)
@pytest.mark.parametrize("blueprint", ["trained", "imported"])
def test_custom_table_with_matrices_equals_the_model(gpu, blueprint, iterations):
    """chance16_mid with its mid-tree chance state at depth 1, D = 3: non-uniform matrices, an infoset payoff_ref and RP_NO_INFO; the
    origins 0, ENTRY and NONE side by side"""
    b = bench("chance16_mid", blueprint)
    fr = b.frontiers(3)
    origin = [(0, ENTRY, NONE)[i % 3] if i % 5 == 4 else 0 for i in range(len(b.entries))]
    results, rows = check_against_model(b, fr, b.entries, origin, iterations, b.labels)
    assert not results["status"].any()
    if iterations == 64:
        assert results["frontiers"][:3].min() > 0 and (rows["kind"] == 1).any()
        assert (b.bp.rows["payoff"] != 0).any()  # the infoset payoff_ref reads something


def test_known_answer_on_the_device(gpu):
    """tests/test_mccfr_depth_model.py's table: the frontier is worth min_j mean_k M[k][j] = -0.5, so c = -0.4 moves the refined policy
    to the terminal and c = -0.6 to the frontier, at the model's iteration count, for its eight seeds, bit for bit"""
    import test_mccfr_depth_model as T

    for c, right in ((-0.4, 0), (-0.6, 1)):
        g, table, fr, entry, rows0 = C.known_answer(c)
        solver = Solver(g, batch=1)
        C.set_frontiers(solver, fr)
        bp = M.Blueprint(table, solver.export())
        assert not bp.rows["weight"].any() and not bp.rows["payoff"].any()
        for seed in T.SEEDS:
            results, rows = solver.depth_solve(entry, 0, iterations=T.ITERATIONS, seed=seed, rows_cap=4)
            D.compare(results[0], rows[0], D.solve(table, bp, fr, entry, 0, iterations=T.ITERATIONS, seed=seed), 4)
            assert results["refined"][0][right] >= 0.75, (c, seed, results["refined"][0][:2])


# ---- invariances: device against device ----
def depth(b, entries, origin, iterations, first_id=FIRST_ID):
    return b.solver.depth_solve(entries, origin, iterations=iterations, seed=SEED, first_id=first_id, rows_cap=ROWS_CAP)


def test_origin_none_is_the_subgame_solve(gpu):
    """origin NONE == rp_mccfr_subgame_solve's bytes; Leduc's origin 1 (no state is deeper) the same; Kuhn and RPS, which keep
    depth() = 0, under any origin"""
    b = bench("leduc", "trained")
    b.frontiers(4)
    safe = b.solver.subgame_solve(b.entries, iterations=64, seed=SEED, first_id=FIRST_ID, rows_cap=ROWS_CAP)
    for origin in (NONE, 1, 7):
        got = depth(b, b.entries, origin, 64)
        assert got[0].tobytes() == safe[0].tobytes() and got[1].tobytes() == safe[1].tobytes(), origin
    assert not safe[0]["frontiers"].any() and not safe[1]["kind"].any()
    k = bench("kuhn", "trained")
    C.set_frontiers(k.solver, C.builtin_frontiers(k.game, 2))
    safe = k.solver.subgame_solve(k.entries, iterations=64, seed=SEED, first_id=FIRST_ID, rows_cap=ROWS_CAP)
    for origin in (None, 0, 3, NONE):
        got = depth(k, k.entries, origin, 64)
        assert got[0].tobytes() == safe[0].tobytes() and got[1].tobytes() == safe[1].tobytes(), origin
    rps = Game("rps")
    solver = Solver(rps, batch=1, seed=1).solve(500)
    C.set_frontiers(solver, C.builtin_frontiers(rps, 3))
    entries = np.array([C.table_entry(s, external, W) for s in (0, 1) for external in (0, 1) for W in (1, 2)], SUBGAME_ENTRY_DTYPE)
    safe = solver.subgame_solve(entries, iterations=7, seed=SEED, rows_cap=8)
    for origin in (None, 0, NONE):
        got = solver.depth_solve(entries, origin, iterations=7, seed=SEED, rows_cap=8)
        assert got[0].tobytes() == safe[0].tobytes() and got[1].tobytes() == safe[1].tobytes() and not got[0]["status"].any()


def test_a_short_solve_is_the_start_of_a_long_one(gpu):
    b = bench("leduc", "trained")
    fr = b.frontiers(2)
    long = D.WithOrigin(b.table, b.bp, fr, b.entries[0], 0, 0, seed=SEED, first_id=FIRST_ID)
    stopped = D.WithOrigin(b.table, b.bp, fr, b.entries[0], 0, 0, seed=SEED, first_id=FIRST_ID)
    for _ in range(64):
        long.step()
    for _ in range(24):
        stopped.step()
    assert [[(n.state, n.kind) for n in t] for t in stopped.trees] == [[(n.state, n.kind) for n in t] for t in long.trees[:24]]
    short, short_rows = depth(b, b.entries[:1], 0, 24)
    D.compare(short[0], short_rows[0], stopped.harvest(), ROWS_CAP)
    got, got_rows = depth(b, b.entries[:1], 0, 64)
    D.compare(got[0], got_rows[0], long.harvest(), ROWS_CAP)


def mixed(b):
    """64 solves: the cases in turn under origin 0, every seventh one malformed, every fifth at another origin"""
    bad = K.malformed(b.entries[1], b.table)
    entries, origin, statuses = [], [], []
    for i in range(64):
        status, e = bad[(i // 7) % len(bad)] if i % 7 == 3 else (M.OK, b.entries[i % len(b.entries)])
        entries.append(e)
        statuses.append(status)
        origin.append((ENTRY, NONE, 1)[i % 3] if i % 5 == 2 else 0)
    return np.array(entries, SUBGAME_ENTRY_DTYPE), np.array(origin, np.uint8), statuses


def test_batch_with_malformed_entries_split_and_reversed(gpu):
    b = bench("leduc", "trained")
    fr = b.frontiers(4)
    entries, origin, statuses = mixed(b)
    whole, whole_rows = check_against_model(b, fr, entries, origin, 7)
    assert list(whole["status"]) == statuses
    head, head_rows = depth(b, entries[:1], origin[:1], 7)
    tail, tail_rows = depth(b, entries[1:], origin[1:], 7, first_id=FIRST_ID + 1)
    assert np.concatenate([head, tail]).tobytes() == whole.tobytes()
    assert np.concatenate([head_rows, tail_rows]).tobytes() == whole_rows.tobytes()
    # reversed in one call: ids are positional, so solve j is the entry 63 - j under id FIRST_ID + j, whatever surrounds it
    flipped, flipped_origin = entries[::-1].copy(), origin[::-1].copy()
    back, back_rows = depth(b, flipped, flipped_origin, 7)
    for j in range(0, 64, 3):
        one, one_rows = depth(b, flipped[j:j + 1], flipped_origin[j:j + 1], 7, first_id=FIRST_ID + j)
        assert one.tobytes() == back[j:j + 1].tobytes() and one_rows.tobytes() == back_rows[j:j + 1].tobytes(), j
    again, again_rows = depth(b, entries, origin, 7)
    assert again.tobytes() == whole.tobytes() and again_rows.tobytes() == whole_rows.tobytes()


def test_the_answer_does_not_depend_on_the_segment_length(gpu):
    """64 iterations in launches of 3 (Pick rows cross launches) and of 64 against the default; RP_MCCFR_SUBGAME_SEGMENT is read by
    every call"""
    b = bench("leduc", "trained")
    b.frontiers(4)
    entries, origin, _ = mixed(b)
    outs = []
    saved = os.environ.pop("RP_MCCFR_SUBGAME_SEGMENT", None)
    try:
        for segment in (None, "3", "64"):
            if segment:
                os.environ["RP_MCCFR_SUBGAME_SEGMENT"] = segment
            results, rows = depth(b, entries[:16], origin[:16], 64)
            outs.append(results.tobytes() + rows.tobytes())
    finally:
        os.environ.pop("RP_MCCFR_SUBGAME_SEGMENT", None)
        if saved is not None:
            os.environ["RP_MCCFR_SUBGAME_SEGMENT"] = saved
    assert (rows["kind"] == 1).any() and results["frontiers"].max() > 3 and results["iterations"][0] == 64
    assert outs[0] == outs[1] == outs[2]


def test_host_form_equals_device_form_and_the_blueprint_is_untouched(gpu):
    b = bench("leduc", "trained")
    before = (b.solver.export().tobytes(), b.solver.epoch, b.solver.counters())
    b.frontiers(2)
    entries, origin, _ = mixed(b)
    host, host_rows = depth(b, entries, origin, 7)
    dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
    d_entries, d_origin = dev(entries), dev(origin)
    d_results = torch.zeros(host.nbytes, dtype=torch.uint8, device="cuda")
    d_rows = torch.zeros(host_rows.nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    b.solver.depth_solve_device(64, d_entries.data_ptr(), d_results.data_ptr(), d_rows.data_ptr(), d_origin.data_ptr(), iterations=7, seed=SEED,
                                first_id=FIRST_ID, rows_cap=ROWS_CAP)
    b.solver.sync()
    assert d_results.cpu().numpy().tobytes() == host.tobytes() and d_rows.cpu().numpy().tobytes() == host_rows.tobytes()
    assert (b.solver.export().tobytes(), b.solver.epoch, b.solver.counters()) == before


# ---- statuses and refusals ----
def test_no_frontier_tables_is_refused_and_set_frontiers_validates_against_the_table(gpu):
    g = Game("leduc")
    solver = Solver(g, batch=1)
    entry = games.depth_entry(g, (4, 1), (), 0)
    with pytest.raises(_lib.RpError, match="no frontier tables"):
        solver.depth_solve(entry, 0)
    f = games.frontiers(g)
    solver.set_frontiers(f["depth"], f["pick_info"], f["payoff_ref"], leaves=2)
    assert solver.depth_solve(entry, 0, iterations=4)[0]["frontiers"][0] > 0
    board = int(np.flatnonzero(f["pick_info"] != _lib.RP_NO_INFO)[0])
    for word, change in (("pick_info", dict(n_pick=int(f["pick_info"][board]))), ("payoff_ref", dict(payoff_ref=(board, g.table.n_infos))),
                         ("payoff_ref", dict(payoff_ref=(board, 0x80000000))), ("payoff_ref", dict(payoff_ref=(0, 0x80000001))),
                         ("leaves", dict(leaves=5))):
        depth_, pick, ref = f["depth"].copy(), f["pick_info"].copy(), f["payoff_ref"].copy()
        if "payoff_ref" in change:
            ref[change["payoff_ref"][0]] = change["payoff_ref"][1]
        with pytest.raises((_lib.RpError, ValueError), match=word):
            solver.set_frontiers(depth_, pick, ref, leaves=change.get("leaves", 2), n_pick=change.get("n_pick"))
        assert solver.depth_solve(entry, 0, iterations=4)[0]["frontiers"][0] > 0  # a refused call leaves the earlier tables
    ref = f["payoff_ref"].copy()
    ref[board] = 0x80000000  # named by one matrix: accepted
    solver.set_frontiers(f["depth"], f["pick_info"], ref, np.ones((1, 2, 2), np.float32), leaves=2)
    solver.set_frontiers(None)  # cleared
    with pytest.raises(_lib.RpError, match="no frontier tables"):
        solver.depth_solve(entry, 0)


def test_a_tree_of_frontiers_overflows_and_the_row_limit_is_a_status(gpu):
    g, table, fr, entry = C.overflowing()
    solver = Solver(g, batch=1)
    C.set_frontiers(solver, fr)
    bp = M.Blueprint(table, solver.export())
    for origin, iterations, status in ((0, 1, M.OK), (0, 2, M.TREE), (NONE, 2, M.OK)):
        results, rows = solver.depth_solve(entry, origin, iterations=iterations, seed=SEED, rows_cap=4)
        want = D.solve(table, bp, fr, entry, origin, iterations=iterations, seed=SEED)
        assert want["status"] == status
        D.compare(results[0], rows[0], want, 4)
    # RP_MSUB_ROWS: test_gpu_mccfr_subgame.py's 1 744-pair table under the depth call; the 1 025th row ends the solve
    wide = game_tables.TableGame(2, [("act", 1, 15), ("act", 0, 14), ("act", 1, 1), ("act", 0, 1)])
    solver, table = Solver(wide, batch=1), M.Table(wide.table)
    fr = C.flat_frontiers(table)
    C.set_frontiers(solver, fr)
    bp = M.Blueprint(table, solver.export())
    entry = C.table_entry(0, external=0, n_worlds=4)
    for iterations, status in ((100, M.OK), (300, M.ROWS)):
        results, rows = solver.depth_solve(entry, 0, iterations=iterations, seed=SEED, rows_cap=4)
        want = D.solve(table, bp, fr, entry, 0, iterations=iterations, seed=SEED)
        assert want["status"] == status
        D.compare(results[0], rows[0], want, 4)


# ---- more solves than one launch takes ----
MS_MAX_CHUNK = 2048  # solves per launch (robopoker_amd/csrc/mccfr_subgame.hpp)


def cycle(b, n):
    """n solves: the cases in turn under origin 0, every seventh one malformed, every fifth at another origin"""
    bad = K.malformed(b.entries[1], b.table)
    entries = [bad[(i // 7) % len(bad)][1] if i % 7 == 3 else b.entries[i % len(b.entries)] for i in range(n)]
    origin = [(NONE, ENTRY, 1)[i % 3] if i % 5 == 0 else 0 for i in range(n)]  # solve 0 without frontiers: not what the last one wants
    return np.array(entries, SUBGAME_ENTRY_DTYPE), np.array(origin, np.uint8)


def test_one_solve_more_than_a_launch_chunk(gpu):
    """2 049 Leduc solves of 7 iterations with frontiers: the second launch chunk holds one solve, whose local profile (Pick rows
    included) lies where solve 0 of the first chunk left its own; in launches of 3 + 3 + 1 iterations the profiles also cross launches.
    The handle is a new one, so that its profile region grows from the 5 solves of the first call to the 2 048 of a full chunk."""
    b = bench("leduc", "trained")
    n, cap, first_id = MS_MAX_CHUNK + 1, 4, 1000
    entries, origin = cycle(b, n)
    assert origin[MS_MAX_CHUNK] == 0 and origin[0] == NONE and {0, ENTRY, NONE} <= set(origin)
    solver = Solver(b.game, "floored", "linear", "external", batch=1, seed=3)
    solver.load_rows(b.solver.export(), b.solver.epoch)
    assert solver.export().tobytes() == b.solver.export().tobytes()
    fr = C.builtin_frontiers(b.game, 4)
    C.set_frontiers(solver, fr)
    run = lambda at, end, first: solver.depth_solve(entries[at:end], origin[at:end], iterations=7, seed=SEED, first_id=first, rows_cap=cap)
    both = lambda out: out[0].tobytes() + out[1].tobytes()
    saved = os.environ.pop("RP_MCCFR_SUBGAME_SEGMENT", None)
    try:
        few = run(0, 5, first_id)
        os.environ["RP_MCCFR_SUBGAME_SEGMENT"] = "3"
        whole = run(0, n, first_id)  # the region grows
        again = run(0, n, first_id)  # both chunks start in what the call before left there
        dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
        d_entries, d_origin = dev(entries), dev(origin)
        d_results, d_rows = (torch.zeros(x.nbytes, dtype=torch.uint8, device="cuda") for x in whole)
        torch.cuda.synchronize()
        solver.depth_solve_device(n, d_entries.data_ptr(), d_results.data_ptr(), d_rows.data_ptr(), d_origin.data_ptr(), iterations=7, seed=SEED,
                                  first_id=first_id, rows_cap=cap)
        solver.sync()
        head, tail = run(0, MS_MAX_CHUNK, first_id), run(MS_MAX_CHUNK, n, first_id + MS_MAX_CHUNK)
        unshifted = run(MS_MAX_CHUNK, n, first_id)
        os.environ.pop("RP_MCCFR_SUBGAME_SEGMENT")
        one_launch_per_chunk = run(0, n, first_id)
    finally:
        os.environ.pop("RP_MCCFR_SUBGAME_SEGMENT", None)
        if saved is not None:
            os.environ["RP_MCCFR_SUBGAME_SEGMENT"] = saved
    results, rows = whole
    last = results[MS_MAX_CHUNK]
    assert last["status"] == M.OK and last["n_actions"] > 1 and last["n_rows"] > 1 and last["frontiers"] > 0 and last["iterations"] == 7
    assert len(set(results["status"])) > 3 and few[0].tobytes() == results[:5].tobytes() and few[1].tobytes() == rows[:5].tobytes()
    for f in (0, 1):
        assert np.concatenate([head[f], tail[f]]).tobytes() == whole[f].tobytes(), ("results", "rows")[f]
    assert both(again) == both(whole) == both(one_launch_per_chunk)
    assert d_results.cpu().numpy().tobytes() == results.tobytes() and d_rows.cpu().numpy().tobytes() == rows.tobytes()
    assert unshifted[0].tobytes() != tail[0].tobytes()  # the id matters
    want = D.solve(b.table, b.bp, fr, entries[MS_MAX_CHUNK], 0, index=MS_MAX_CHUNK, iterations=7, seed=SEED, first_id=first_id)
    D.compare(last, rows[MS_MAX_CHUNK], want, cap)

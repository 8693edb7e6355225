"""Host mirror of the reference's ``mccfr::Solver`` surface over the MI355X C-ABI.

Names and meaning follow crates/mccfr/src/solver/solver.rs (``step``, ``solve``, ``spend``,
``exploitability``) and strategy/profile.rs (``t`` -> ``epoch``, ``cum_*`` -> ``get``,
``iterated_distribution`` / ``averaged_distribution`` -> ``policy``).  All compute happens in
librp_mi355x.so's HIP kernels; there is no CPU path here.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .games import Game

ENC_DTYPE = np.dtype([("weight", "<f4"), ("regret", "<f4"), ("payoff", "<f4"), ("visits", "<u4")])
# the safe subgame re-solve's records (include/rp_mi355x.h: rp_mccfr_subgame_prior 104, _entry 140, _result 192, _row 264 bytes)
SUBGAME_PRIOR_DTYPE = np.dtype([("root_state", "<u4", 16), ("secret", "u1", 16), ("path", "u1", 16), ("n_prior", "u1"), ("n_path", "u1"),
                                ("internal", "u1"), ("mode", "u1"), ("n_worlds", "u1"), ("pad", "u1", 3)])
SUBGAME_ENTRY_DTYPE = np.dtype([("observed", "<u4"), ("harvest_info", "<u4"), ("candidate", "<u4", 16), ("secret", "u1", 16),
                                ("world_of", "u1", 16), ("harvest_order", "u1", 16), ("weights", "<f4", 4), ("external", "u1"),
                                ("n_candidates", "u1"), ("n_worlds", "u1"), ("pad", "u1")])
SUBGAME_RESULT_DTYPE = np.dtype([("info", "<u4"), ("n_actions", "u1"), ("status", "u1"), ("pad", "u1", 2), ("refined", "<f4", 16),
                                 ("visits", "<u4", 16), ("regret", "<f4"), ("sum_regret", "<f4"), ("iterations", "<u4"), ("n_rows", "<u4"),
                                 ("nodes", "<u8"), ("infosets", "<u8"), ("drawn", "<u4", 4), ("fallbacks", "<u4"), ("frontiers", "<u4")])
SUBGAME_ROW_DTYPE = np.dtype([("world", "u1"), ("n_actions", "u1"), ("kind", "u1"), ("pad", "u1"), ("info", "<u4"), ("enc", ENC_DTYPE, 16)])
assert (SUBGAME_PRIOR_DTYPE.itemsize, SUBGAME_ENTRY_DTYPE.itemsize, SUBGAME_RESULT_DTYPE.itemsize, SUBGAME_ROW_DTYPE.itemsize) == (104, 140, 192, 264)


def default_hyper() -> _lib.Hyper:
    hp = _lib.Hyper()
    _lib.load().rp_hyper_default(C.byref(hp))
    return hp


class Solver:
    """``mccfr!(..)<R, W, S>`` (strategy/macros.rs:7-151) on one MI355X.

    Parameters mirror the reference's type parameters: ``regret`` = RegretSchedule, ``weight`` =
    WeightSchedule, ``sampling`` = SamplingScheme, ``batch`` = ``Solver::batch_size()``.
    """

    def __init__(self, game: Game, regret="floored", weight="linear", sampling="external", batch=1, seed=0,
                 hyper=None, device=0, mode=None):
        self._lib = _lib.load()
        self.game = game
        self.hp = hyper if hyper is not None else default_hyper()
        self._h = C.c_void_p()
        if mode is None:  # the reference's exact order (rp_mccfr_create's default)
            _lib.check(self._lib.rp_mccfr_create(C.byref(game.table), _lib.REGRET[regret], _lib.WEIGHT[weight],
                                                 _lib.SAMPLING[sampling], batch, C.byref(self.hp), seed, device,
                                                 C.byref(self._h)))
        else:
            _lib.check(self._lib.rp_mccfr_create_mode(C.byref(game.table), _lib.REGRET[regret], _lib.WEIGHT[weight],
                                                      _lib.SAMPLING[sampling], batch, C.byref(self.hp), seed, device,
                                                      _lib.UPDATE[mode], C.byref(self._h)))
        self.batch = batch
        self.cells = game.table.n_infos * game.table.max_actions

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rp_mccfr_destroy(self._h)
            self._h = None

    __del__ = close

    # ---- Solver ---------------------------------------------------------------------------------
    def step(self):
        _lib.check(self._lib.rp_mccfr_step(self._h))

    def step_async(self, steps=1):
        _lib.check(self._lib.rp_mccfr_step_async(self._h, steps))

    def sync(self):
        _lib.check(self._lib.rp_mccfr_sync(self._h))

    def solve(self, trees: int):
        _lib.check(self._lib.rp_mccfr_solve(self._h, trees))
        return self

    def spend(self, seconds: float):
        it, el = C.c_uint64(), C.c_double()
        _lib.check(self._lib.rp_mccfr_spend(self._h, seconds, C.byref(it), C.byref(el)))
        return it.value, el.value

    def train(self, max_steps=0, max_seconds=0.0, log_interval=60.0, flush_interval=1800.0, on_checkpoint=None,
              on_flush=None, interrupt=None):
        """``Trainer::train`` (crates/forge/src/trainer.rs:18-66): loop { step; checkpoint; flush; interrupt? } in the
        library.  ``on_checkpoint(dict, line)`` gets the Checkpoint and its display line, ``on_flush(dict)`` fires at
        the flush cadence, ``interrupt`` is a ctypes c_int the caller may set to stop.  Returns Progress::summary."""
        return _lib.train(self._lib.rp_mccfr_train, self._h, max_steps=max_steps, max_seconds=max_seconds, log_interval=log_interval,
                          flush_interval=flush_interval, on_checkpoint=on_checkpoint, on_flush=on_flush, interrupt=interrupt)

    def exploitability(self) -> float:
        out = C.c_float()
        _lib.check(self._lib.rp_mccfr_exploitability(self._h, C.byref(out)))
        return out.value

    # ---- CfrNash on the device (csrc/mccfr_nash.hpp): the same bits as exploitability(), in stream order --------------------------
    def exploitability_device(self, out_dev_ptr: int):
        """queues the best response on the solver's stream; one f32 lands at ``out_dev_ptr`` (device memory), no host sync"""
        _lib.check(self._lib.rp_mccfr_exploitability_device(self._h, C.c_void_p(out_dev_ptr)))

    def best_response(self) -> dict:
        """``exploitability`` with its parts: ``values`` [n_players] (optimal_response_payoff), ``choice`` [n_infos]
        (optimal_cfactual_choice, the action slot), ``cfv`` [n_infos, max_actions] (optimal_cfactual_payoff)"""
        t = self.game.table
        e = C.c_float()
        values = np.zeros(t.n_players, dtype=np.float32)
        choice = np.zeros(t.n_infos, dtype=np.uint8)
        cfv = np.zeros((t.n_infos, t.max_actions), dtype=np.float32)
        _lib.check(self._lib.rp_mccfr_best_response(self._h, C.byref(e), values.ctypes.data_as(C.POINTER(C.c_float)),
                                                    choice.ctypes.data_as(C.POINTER(C.c_uint8)), cfv.ctypes.data_as(C.POINTER(C.c_float))))
        return {"exploitability": np.float32(e.value), "values": values, "choice": choice, "cfv": cfv}

    def nash_variant(self) -> str:
        """the launch shape of the device best response: "one" (one workgroup per hero, LDS) or "levels" (a launch per level)"""
        v = C.c_int()
        _lib.check(self._lib.rp_mccfr_nash_variant(self._h, C.byref(v)))
        return ("one", "levels")[v.value]

    def solve_to(self, target: float, check_every: int, max_steps: int):
        """step in blocks of ``check_every`` until the first device check below ``target`` or ``max_steps``;
        returns (steps, exploitability, reached)"""
        steps, e, hit = C.c_uint64(), C.c_float(), C.c_int()
        _lib.check(self._lib.rp_mccfr_solve_to(self._h, target, check_every, max_steps, C.byref(steps), C.byref(e), C.byref(hit)))
        return steps.value, e.value, bool(hit.value)

    # ---- RefProf / MutProf ----------------------------------------------------------------------
    @property
    def epoch(self) -> int:
        e = C.c_uint64()
        _lib.check(self._lib.rp_mccfr_epoch(self._h, C.byref(e)))
        return e.value

    def counters(self):
        a, b = C.c_uint64(), C.c_uint64()
        _lib.check(self._lib.rp_mccfr_counters(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def get(self, info: int, edge: int) -> _lib.Encounter:
        e = _lib.Encounter()
        _lib.check(self._lib.rp_mccfr_get(self._h, info, edge, C.byref(e)))
        return e

    def set(self, info: int, edge: int, weight=0.0, regret=0.0, payoff=0.0, visits=0):
        e = _lib.Encounter(weight, regret, payoff, visits)
        _lib.check(self._lib.rp_mccfr_set(self._h, info, edge, C.byref(e)))

    def export(self) -> np.ndarray:
        rows = np.zeros(self.cells, dtype=ENC_DTYPE)
        _lib.check(self._lib.rp_mccfr_export(self._h, rows.ctypes.data_as(C.POINTER(_lib.Encounter)), self.cells))
        return rows

    def load_rows(self, rows: np.ndarray, epoch: int):
        buf = np.ascontiguousarray(rows, dtype=ENC_DTYPE)
        _lib.check(self._lib.rp_mccfr_import(self._h, buf.ctypes.data_as(C.POINTER(_lib.Encounter)), buf.size, epoch))

    def policy(self, info: int, kind="averaged") -> np.ndarray:
        out = (C.c_float * 16)()
        n = C.c_uint32()
        _lib.check(self._lib.rp_mccfr_policy(self._h, info, _lib.DIST[kind], out, C.byref(n)))
        return np.array(out[: n.value], dtype=np.float32)

    def sum_regret(self) -> float:
        out = C.c_float()
        _lib.check(self._lib.rp_mccfr_sum_regret(self._h, C.byref(out)))
        return out.value

    # ---- the safe subgame re-solve with this solver's tables as the blueprint (csrc/mccfr_subgame.hpp); read-only on the solver -------
    def subgame_args(self, iterations=1, prior=float(1 << 14), seed=0, first_id=0, rows_cap=0) -> _lib.MccfrSubgameArgs:
        a = _lib.MccfrSubgameArgs()
        self._lib.rp_mccfr_subgame_args_default(C.byref(a))
        a.iterations, a.prior, a.seed, a.first_id, a.rows_cap = iterations, prior, seed, first_id, rows_cap
        return a

    def subgame_belief(self, priors: np.ndarray) -> dict:
        """``Posterior`` -> ``partition::<W>`` per entry of ``priors`` (SUBGAME_PRIOR_DTYPE; games.subgame_entry builds them):
        {"world_of" [n, 16] u8, "weights" [n, 4] f32, "status" [n] u8}"""
        buf = np.ascontiguousarray(priors, dtype=SUBGAME_PRIOR_DTYPE).reshape(-1)
        n = buf.size
        out = {"world_of": np.zeros((n, 16), np.uint8), "weights": np.zeros((n, 4), np.float32), "status": np.zeros(n, np.uint8)}
        _lib.check(self._lib.rp_mccfr_subgame_belief(self._h, n, buf.ctypes.data, out["world_of"].ctypes.data, out["weights"].ctypes.data,
                                                     out["status"].ctypes.data))
        return out

    def subgame_belief_device(self, n: int, priors_ptr: int, world_of_ptr: int, weights_ptr: int, status_ptr: int = 0):
        """the same, every array in device memory; queued on the solver's stream, no host synchronisation"""
        _lib.check(self._lib.rp_mccfr_subgame_belief_device(self._h, n, priors_ptr, world_of_ptr, weights_ptr, status_ptr or None))

    def subgame_solve(self, entries: np.ndarray, iterations=1, prior=float(1 << 14), seed=0, first_id=0, rows_cap=0):
        """``SubGameSolver`` (origin = None) x ``iterations`` and its harvest, one solve per entry (SUBGAME_ENTRY_DTYPE):
        (results [n] SUBGAME_RESULT_DTYPE, rows [n, rows_cap] SUBGAME_ROW_DTYPE)"""
        buf = np.ascontiguousarray(entries, dtype=SUBGAME_ENTRY_DTYPE).reshape(-1)
        n = buf.size
        results, rows = np.zeros(n, SUBGAME_RESULT_DTYPE), np.zeros((n, rows_cap), SUBGAME_ROW_DTYPE)
        a = self.subgame_args(iterations, prior, seed, first_id, rows_cap)
        _lib.check(self._lib.rp_mccfr_subgame_solve(self._h, n, buf.ctypes.data, C.byref(a), results.ctypes.data,
                                                    rows.ctypes.data if rows_cap else None))
        return results, rows

    def subgame_solve_device(self, n: int, entries_ptr: int, results_ptr: int, rows_ptr: int = 0, **args):
        """the same, every array in device memory (``args`` as subgame_args); queued on the solver's stream, no host synchronisation"""
        a = self.subgame_args(**args)
        _lib.check(self._lib.rp_mccfr_subgame_solve_device(self._h, n, entries_ptr, C.byref(a), results_ptr, rows_ptr or None))

    # ---- the depth-limited re-solve (SubGameSolver::with_origin, DepthSolver) over the same records; read-only on the solver ------------
    def set_frontiers(self, depth=None, pick_info=None, payoff_ref=None, matrices=None, leaves=4, n_pick=None):
        """rp_mccfr_set_frontiers: per state ``depth`` (u8), ``pick_info`` and ``payoff_ref`` (u32; games.frontiers answers the three
        for a built-in game), ``matrices`` [m, leaves, leaves] f32 named by payoff_ref 0x80000000 | m.  ``n_pick`` defaults to
        the largest pick id + 1.  ``depth=None`` clears."""
        if depth is None:
            _lib.check(self._lib.rp_mccfr_set_frontiers(self._h, None))
            return
        depth = np.ascontiguousarray(depth, np.uint8)
        pick_info, payoff_ref = np.ascontiguousarray(pick_info, np.uint32), np.ascontiguousarray(payoff_ref, np.uint32)
        n = self.game.table.n_states
        if not depth.shape == pick_info.shape == payoff_ref.shape == (n,):
            raise ValueError(f"depth, pick_info and payoff_ref hold one element per state ({n})")
        mats = np.zeros((0, leaves, leaves), np.float32) if matrices is None else np.ascontiguousarray(matrices, np.float32)
        if mats.ndim != 3 or mats.shape[1:] != (leaves, leaves):
            raise ValueError("matrices is [m, leaves, leaves]")
        if n_pick is None:
            picks = pick_info[pick_info != _lib.RP_NO_INFO]
            n_pick = int(picks.max()) + 1 if picks.size else 0
        f = _lib.MccfrFrontiers(depth.ctypes.data, pick_info.ctypes.data, payoff_ref.ctypes.data, mats.ctypes.data if len(mats) else None,
                                n_pick, len(mats), leaves, 0)
        _lib.check(self._lib.rp_mccfr_set_frontiers(self._h, C.byref(f)))

    @staticmethod
    def _origin(origin, n):
        """-> uint8[n] or None (the whole batch at RP_MCCFR_ORIGIN_ENTRY); a None among per-entry origins reads as ORIGIN_ENTRY"""
        if origin is None:
            return None
        if np.isscalar(origin):
            origin = [origin] * n
        o = np.array([_lib.RP_MCCFR_ORIGIN_ENTRY if x is None else x for x in origin], np.uint8)
        if o.shape != (n,):
            raise ValueError(f"{n} entries, {o.size} origins")
        return o

    def depth_solve(self, entries: np.ndarray, origin=None, iterations=1, prior=float(1 << 14), seed=0, first_id=0, rows_cap=0):
        """``SubGameSolver::with_origin(origin)`` x ``iterations`` and its harvest, one solve per entry (SUBGAME_ENTRY_DTYPE;
        games.depth_entry builds the ``DepthSolver`` form).  ``origin``: None = every entry at its own depth (ORIGIN_ENTRY), a number
        or one per entry (0 .. 253, ORIGIN_ENTRY, ORIGIN_NONE).  -> (results [n] SUBGAME_RESULT_DTYPE, rows [n, rows_cap]
        SUBGAME_ROW_DTYPE sorted by (world, kind, info)).  Needs set_frontiers."""
        buf = np.ascontiguousarray(entries, dtype=SUBGAME_ENTRY_DTYPE).reshape(-1)
        n = buf.size
        o = self._origin(origin, n)
        results, rows = np.zeros(n, SUBGAME_RESULT_DTYPE), np.zeros((n, rows_cap), SUBGAME_ROW_DTYPE)
        a = self.subgame_args(iterations, prior, seed, first_id, rows_cap)
        _lib.check(self._lib.rp_mccfr_depth_solve(self._h, n, buf.ctypes.data, o.ctypes.data if o is not None else None, C.byref(a),
                                                  results.ctypes.data, rows.ctypes.data if rows_cap else None))
        return results, rows

    def depth_solve_device(self, n: int, entries_ptr: int, results_ptr: int, rows_ptr: int = 0, origin_ptr: int = 0, **args):
        """the same, every array in device memory (``args`` as subgame_args); queued on the solver's stream, no host synchronisation"""
        a = self.subgame_args(**args)
        _lib.check(self._lib.rp_mccfr_depth_solve_device(self._h, n, entries_ptr, origin_ptr or None, C.byref(a), results_ptr, rows_ptr or None))

    # ---- knobs ----------------------------------------------------------------------------------
    def set_batch(self, batch: int):
        _lib.check(self._lib.rp_mccfr_set_batch(self._h, batch))
        self.batch = batch

    def set_update_mode(self, mode: str):
        _lib.check(self._lib.rp_mccfr_set_update_mode(self._h, _lib.UPDATE[mode]))

    def set_rng(self, kind: str, streams: "_lib.HashStreams | None" = None):
        """"counter" (default: the build's own hash) or "reference" (the reference's DefaultHasher -> SmallRng chain,
        include/rp_refrng.h); `streams` defaults to the built-in game's (Game.hash_streams)"""
        if kind == "reference" and streams is None:
            streams = self.game.hash_streams()
        _lib.check(self._lib.rp_mccfr_set_rng(self._h, _lib.RNG[kind], C.byref(streams) if streams is not None else None))

    def set_stream(self, hip_stream_ptr):
        _lib.check(self._lib.rp_mccfr_set_stream(self._h, C.c_void_p(hip_stream_ptr)))

    # ---- multi-GPU exchange --------------------------------------------------------
    def set_shard(self, rank: int, world: int):
        _lib.check(self._lib.rp_mccfr_set_shard(self._h, rank, world))

    def summary_bytes(self) -> int:
        n = C.c_size_t()
        _lib.check(self._lib.rp_mccfr_summary_bytes(self._h, C.byref(n)))
        return n.value

    def step_local(self, summary_dev_ptr: int):
        _lib.check(self._lib.rp_mccfr_step_local(self._h, C.c_void_p(summary_dev_ptr)))

    def step_apply(self, gathered_dev_ptr: int, world: int):
        _lib.check(self._lib.rp_mccfr_step_apply(self._h, C.c_void_p(gathered_dev_ptr), world))

    def window_local(self, window_dev_ptr: int, first: bool):
        _lib.check(self._lib.rp_mccfr_window_local(self._h, C.c_void_p(window_dev_ptr), 1 if first else 0))

    def window_apply(self, gathered_dev_ptr: int, world: int):
        _lib.check(self._lib.rp_mccfr_window_apply(self._h, C.c_void_p(gathered_dev_ptr), world))

    def step_comm(self, comm, steps: int, window: int = 1):
        """``steps`` sharded steps over an ``rp_comm`` (robopoker_amd.parallel.Comm): exchange windows of ``window`` local
        steps, one ncclAllGather per window on the solver's stream, no host work in between"""
        _lib.check(self._lib.rp_mccfr_step_comm(self._h, comm.handle, steps, window))

    # ---- profiling hooks ------------------------------------------------------------------------
    def profile(self, enable=True):
        _lib.check(self._lib.rp_mccfr_profile(self._h, 1 if enable else 0))

    def kernel_variant(self) -> str:
        """which Solver::batch kernel runs: "hbm" (any game), "lds" (small games), "static" (compile-time skeleton)"""
        v = C.c_int()
        _lib.check(self._lib.rp_mccfr_traversal_variant(self._h, C.byref(v)))
        return ("hbm", "lds", "static")[v.value]

    def fold_variant(self) -> str:
        """how a composed step of the current batch size folds its group maps: "fused" (inside k_combine2) or "split" (k_fold_groups)"""
        v = C.c_int()
        _lib.check(self._lib.rp_mccfr_fold_variant(self._h, C.byref(v)))
        return ("fused", "split")[v.value]

    def traversal_rows_bytes(self) -> int:
        """size of the packed-row game table of the "static" traversal; 0: it follows the child records (RP_TRAV_NO_FLAT=1)"""
        n = C.c_size_t()
        _lib.check(self._lib.rp_mccfr_traversal_rows_bytes(self._h, C.byref(n)))
        return n.value

    def kernel_time(self, name: str):
        return _lib.kernel_time(self._lib.rp_mccfr_kernel_time, self._h, name)

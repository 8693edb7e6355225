"""The NLHE rules engine on the device (include/rp_mi355x.h, rp_nlhe_playouts; robopoker_amd/csrc/nlhe.hip): random
abstract hands played by the device-side restatement of ``kicker::GameN`` / ``NlheGame::apply`` / ``Showdown::settle``."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch  # before the first HIP call of librp_mi355x.so: one HIP runtime per process

from . import _lib

A = 9  # widest NLHE infoset (pokerkit/src/lib.rs:130-133)
ENC_DTYPE = np.dtype([("weight", "<f4"), ("regret", "<f4"), ("payoff", "<f4"), ("visits", "<u4")])


MAX_HISTORY, MAX_HOLES, BUCKETS = _lib.RP_NLHE_MAX_HISTORY, _lib.RP_NLHE_MAX_HOLES, 256
RECALL_DTYPE = np.dtype([("hole", "<u8"), ("draws", "<u8", (3,)), ("stacks", "<i2", (2,)), ("pov", "u1"), ("dealer", "u1"),
                         ("n_edges", "u1"), ("reserved", "u1"), ("edges", "u1", (MAX_HISTORY,))])  # rp_nlhe_recall, 88 bytes
assert RECALL_DTYPE.itemsize == C.sizeof(_lib.NlheRecall) == 88
MAX_PLAYS = _lib.RP_AIVAT_MAX_PLAYS
AIVAT_DTYPE = np.dtype([("hole", "<u8", (2,)), ("draws", "<u8", (3,)), ("stacks", "<i2", (2,)), ("chips", "<i2", (MAX_PLAYS,)),
                        ("kind", "u1", (MAX_PLAYS,)), ("seat", "u1"), ("dealer", "u1"), ("n_plays", "u1"), ("board_mode", "u1")])  # rp_aivat_hand
assert AIVAT_DTYPE.itemsize == C.sizeof(_lib.AivatHand) == 192
LEAVES, MAX_PREFIX, MAX_ROLLOUTS = _lib.RP_NLHE_FRONTIER_LEAVES, _lib.RP_NLHE_MAX_PREFIX, 4096
FRONTIER_DTYPE = np.dtype([("holes", "<u8", (2,)), ("draws", "<u8", (3,)), ("stacks", "<i2", (2,)), ("internal", "u1"), ("dealer", "u1"),
                           ("n_edges", "u1"), ("n_prefix", "u1"), ("edges", "u1", (MAX_HISTORY,)), ("prefix", "u1", (MAX_PREFIX,)),
                           ("reserved", "u1", (4,))])  # rp_nlhe_frontier, 112 bytes
assert FRONTIER_DTYPE.itemsize == C.sizeof(_lib.NlheFrontier) == 112
DEPTH_RESULT_DTYPE = np.dtype([("past", "<u8"), ("choices", "<u8"), ("present", "<u4"), ("n_actions", "u1"), ("status", "u1"), ("pad", "u1", (2,)),
                               ("refined", "<f4", (A,)), ("visits", "<u4", (A,)), ("regret", "<f4"), ("sum_regret", "<f4"),
                               ("iterations", "<u4"), ("n_rows", "<u4"), ("nodes", "<u8"), ("infosets", "<u8"), ("frontiers", "<u8"),
                               ("rollouts", "<u8")])  # rp_nlhe_depth_result, 144 bytes
DEPTH_ROW_DTYPE = np.dtype([("kind", "u1"), ("n_actions", "u1"), ("pad", "u1", (2,)), ("present", "<u4"), ("past", "<u8"), ("choices", "<u8"),
                            ("enc", ENC_DTYPE, (A,))])  # rp_nlhe_depth_row, 168 bytes
assert DEPTH_RESULT_DTYPE.itemsize == C.sizeof(_lib.NlheDepthResult) == 144 and DEPTH_ROW_DTYPE.itemsize == C.sizeof(_lib.NlheDepthRow) == 168
ORIGIN_ENTRY = _lib.RP_NLHE_DEPTH_ORIGIN_ENTRY
SUBGAME_RESULT_DTYPE = np.dtype(DEPTH_RESULT_DTYPE.descr + [("drawn", "<u4", (4,)), ("attempts", "<u8"), ("fallbacks", "<u4"),
                                                            ("pad2", "<u4")])  # rp_nlhe_subgame_result, 176 bytes
SUBGAME_ROW_DTYPE = np.dtype([("kind", "u1"), ("n_actions", "u1"), ("world", "u1"), ("pad", "u1"), ("present", "<u4"), ("past", "<u8"),
                              ("choices", "<u8"), ("enc", ENC_DTYPE, (A,))])  # rp_nlhe_subgame_row, 168 bytes
SUBGAME_DEAL_DTYPE = np.dtype([("hole", "<u8"), ("world", "u1"), ("pad", "u1"), ("attempts", "<u2"), ("pad2", "<u4")])  # rp_nlhe_subgame_deal
assert SUBGAME_RESULT_DTYPE.itemsize == C.sizeof(_lib.NlheSubgameResult) == 176 and SUBGAME_ROW_DTYPE.itemsize == C.sizeof(_lib.NlheSubgameRow) == 168
assert SUBGAME_DEAL_DTYPE.itemsize == C.sizeof(_lib.NlheSubgameDeal) == 16 and C.sizeof(_lib.NlheSubgameArgs) == 48
ORIGIN_NONE = _lib.RP_NLHE_SUBGAME_ORIGIN_NONE
SEARCH_STEP_DTYPE = np.dtype([("solve_id", "<u8"), ("recall", RECALL_DTYPE), ("result", SUBGAME_RESULT_DTYPE), ("bp", "<f4", (A,)), ("p", "<f4", (A,)),
                              ("decision", "<u4"), ("seat", "u1"), ("edge", "u1"), ("fallback", "u1"),
                              ("belief_status", "u1")])  # rp_nlhe_search_step, 352 bytes
assert SEARCH_STEP_DTYPE.itemsize == C.sizeof(_lib.NlheSearchStep) == 352 and C.sizeof(_lib.NlheSearchArgs) == 72
CENSUS_TOP, CENSUS_SEGMENT, CENSUS_STREETS, CENSUS_CODES = (_lib.RP_NLHE_CENSUS_TOP, _lib.RP_NLHE_CENSUS_SEGMENT, _lib.RP_NLHE_CENSUS_STREETS,
                                                              _lib.RP_NLHE_CENSUS_CODES)
CENSUS_CELL_DTYPE = np.dtype([("rows", "<u8"), ("rated", "<u8"), ("dominant", "<u8"), ("visits", "<u8"), ("ratio", "<f8"), ("weight", "<f8"),
                              ("total", "<f8"), ("regret", "<f8"), ("payoff", "<f8"), ("max_regret", "<f4"), ("min_regret", "<f4"),
                              ("max_weight", "<f4"), ("max_payoff", "<f4"), ("min_payoff", "<f4"), ("max_visits", "<u4"), ("min_visits", "<u4"),
                              ("reserved", "<u4")])  # rp_census_cell, 104 bytes
CENSUS_ENTRY_DTYPE = np.dtype([("past", "<u8"), ("choices", "<u8"), ("present", "<u4"), ("edges", "<u4"), ("visits", "<u4"),
                               ("regret", "<f4")])  # rp_census_entry, 32 bytes
CENSUS_DTYPE = np.dtype([("cell", CENSUS_CELL_DTYPE, (CENSUS_STREETS, CENSUS_CODES)), ("infosets", "<u8", (CENSUS_STREETS,)), ("epoch", "<u8"),
                         ("slots", "<u8"), ("n_cold", "<u4"), ("n_hot", "<u4"), ("cold", CENSUS_ENTRY_DTYPE, (CENSUS_TOP,)),
                         ("hot", CENSUS_ENTRY_DTYPE, (CENSUS_TOP,))])  # rp_census, 20 800 bytes
assert CENSUS_CELL_DTYPE.itemsize == C.sizeof(_lib.CensusCell) == 104 and CENSUS_ENTRY_DTYPE.itemsize == C.sizeof(_lib.CensusEntry) == 32
assert CENSUS_DTYPE.itemsize == C.sizeof(_lib.Census) == 20800
# Edge's Display (kicker/src/edge.rs:229-241) by 5-bit edge code; code 0 is no edge, codes from 20 on name nothing
EDGE_NAMES = ("", "?", "F", "O", "*", "!", "2bb", "3bb", "4bb", "5bb", "1:4", "1:3", "1:2", "2:3", "3:4", "1:1", "5:4", "3:2", "2:1", "3:1")
STREET_NAMES = "PFTR?"


def edge_name(code: int) -> str:
    """``format!("{}", Edge::from(code))``; a code that is no edge reads "#<code>" """
    return EDGE_NAMES[code] if 0 < code < len(EDGE_NAMES) else f"#{code}"


def _census_ptr(census):
    """a census record (``NlheSolver.table_census()``'s, or any CENSUS_DTYPE array of one item) as the summaries' argument"""
    rec = np.ascontiguousarray(census, CENSUS_DTYPE).reshape(-1)
    assert rec.size == 1, "one rp_census record"
    return rec, _p(rec)


def census_stats(census):
    """``TrainingAPI::stats`` (ApiBlueprintStats) of a census record: dict(infosets, edges, avg_/max_/min_regret, avg_/max_weight,
    avg_/max_/min_payoff, avg_/max_/min_visits); float32 where the reference's are.  Host arithmetic, no device."""
    rec, ptr = _census_ptr(census)
    s = _lib.CensusTotals()
    _lib.check(_lib.load().rp_census_stats(ptr, C.byref(s)))
    out = dict(infosets=int(s.infosets), edges=int(s.edges), max_visits=int(s.max_visits), min_visits=int(s.min_visits))
    out.update({k: np.float32(getattr(s, k)) for k in ("avg_regret", "max_regret", "min_regret", "avg_weight", "max_weight", "avg_payoff",
                                                       "max_payoff", "min_payoff", "avg_visits")})
    return out


def census_street_stats(census):
    """``TrainingAPI::street_stats`` (ApiStreetStats): five dicts, street "P" "F" "T" "R" "?", a street without rows all zero"""
    rec, ptr = _census_ptr(census)
    s = (_lib.CensusStreet * CENSUS_STREETS)()
    _lib.check(_lib.load().rp_census_street_stats(ptr, s))
    return [dict(street=x.street.decode(), infosets=int(x.infosets), edges=int(x.edges),
                 **{k: np.float32(getattr(x, k)) for k in ("avg_regret", "avg_weight", "avg_payoff", "avg_visits")}) for x in s]


def census_saturation(census):
    """``TrainingAPI::saturation`` (ApiSaturation): how close the table's largest magnitudes are to f32::MAX"""
    rec, ptr = _census_ptr(census)
    s = _lib.CensusPeaks()
    _lib.check(_lib.load().rp_census_saturation(ptr, C.byref(s)))
    return dict(max_visits=int(s.max_visits), **{k: np.float32(getattr(s, k)) for k in ("max_weight", "max_regret", "max_payoff", "precision_f32",
                                                                                      "weight_pct", "regret_pct")})


def census_grid_usage(census):
    """``StrategyAPI::grid_usage`` (ApiGridUsage): one dict per non-empty (street, edge) cell — street, edge (``Edge``'s display), code,
    avg_freq, weighted_freq, n_decisions_with_edge, n_dominant — by street, then avg_freq descending"""
    rec, ptr = _census_ptr(census)
    rows, n = (_lib.CensusGrid * (CENSUS_STREETS * CENSUS_CODES))(), C.c_uint32()
    _lib.check(_lib.load().rp_census_grid_usage(ptr, rows, C.byref(n)))
    return [dict(street=STREET_NAMES[r.street], edge=edge_name(r.edge), code=int(r.edge), avg_freq=np.float32(r.avg_freq),
                 weighted_freq=np.float32(r.weighted_freq), n_decisions_with_edge=int(r.n_decisions_with_edge), n_dominant=int(r.n_dominant))
            for r in rows[: n.value]]


def census_cold(census, k=CENSUS_TOP):
    """``TrainingAPI::cold(k)`` (ApiColdInfoset), k <= 64: the infosets with the fewest visits of their least visited action"""
    rec = np.ascontiguousarray(census, CENSUS_DTYPE).reshape(-1)[0]
    return [dict(past=int(e["past"]), present=int(e["present"]), choices=int(e["choices"]), visits=int(e["visits"]), edges=int(e["edges"]))
            for e in rec["cold"][: min(int(k), int(rec["n_cold"]))]]


def census_hot(census, k=CENSUS_TOP):
    """``TrainingAPI::hot(k)`` (ApiHotInfoset), k <= 64: the infosets with the largest regret magnitude; max_regret = MAX(regret)"""
    rec = np.ascontiguousarray(census, CENSUS_DTYPE).reshape(-1)[0]
    return [dict(past=int(e["past"]), present=int(e["present"]), choices=int(e["choices"]), max_regret=np.float32(e["regret"]),
                 edges=int(e["edges"])) for e in rec["hot"][: min(int(k), int(rec["n_hot"]))]]


WORLDS, MAX_REJECTIONS, WORLD_NONE, MAX_DEALS = _lib.RP_NLHE_WORLDS, _lib.RP_NLHE_MAX_REJECTIONS, _lib.RP_WORLD_NONE, 4096


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _dptr(t, live):
    """the address of a device tensor for a _device call; NULL where ``live`` is false (nothing to do) or there is no tensor"""
    return C.c_void_p(t.data_ptr()) if live and t is not None else None


def _records(t, dtype):
    """a device uint8 tensor holding packed ``dtype`` records -> (the tensor contiguous, n, its device)"""
    t = t.contiguous()
    assert t.is_cuda and t.element_size() == 1 and t.numel() % dtype.itemsize == 0
    return t, t.numel() // dtype.itemsize, t.device


class Recall:
    """What one seat has seen, at edge level: a ``Witness`` (crates/kicker/src/witness.rs:36-44) after ``Recall::history()``.
    ``hole``: pov's two cards as a mask (bit c = card c); ``draws``: up to three masks (flop, turn, river) in street order;
    ``edges``: edge codes, Draw edges (1) included; ``stacks`` (0, 0) = the reference's STACK.  Nothing is checked here: a
    malformed recall is answered with its status by the queries."""

    def __init__(self, pov, hole, draws=(), edges=(), stacks=(0, 0), dealer=0):
        self.pov, self.hole, self.draws, self.edges, self.stacks, self.dealer = pov, hole, tuple(draws), tuple(edges), tuple(stacks), dealer

    @staticmethod
    def pack(recalls) -> np.ndarray:
        """-> RECALL_DTYPE[n]; a history longer than the cap keeps its first 48 edges and its true length clipped to 255 (status LENGTH)"""
        if isinstance(recalls, np.ndarray) and recalls.dtype == RECALL_DTYPE:
            return np.ascontiguousarray(recalls)
        if isinstance(recalls, Recall):
            recalls = [recalls]
        out = np.zeros(len(recalls), RECALL_DTYPE)
        for i, r in enumerate(recalls):
            out[i]["hole"] = r.hole
            out[i]["draws"][: len(r.draws)] = r.draws
            out[i]["stacks"] = r.stacks
            out[i]["pov"], out[i]["dealer"], out[i]["n_edges"] = r.pov, r.dealer, min(len(r.edges), 255)
            k = min(len(r.edges), MAX_HISTORY)
            out[i]["edges"][:k] = r.edges[:k]
        return out


class AivatHand:
    """One played heads-up hand at ACTION level, as the AIVAT evaluator takes it (crates/arena/src/aivat.rs:63-93): ``holes`` the
    two-card masks of seat 0 and seat 1; ``draws`` up to three masks (flop, turn, river) as dealt; ``plays`` the hand's choice plays
    in order, each (kind, chips) with kind "fold" / "check" / "call" / "raise" / "shove" (or its rp_aivat_play code) and chips the
    amount the play adds (ignored for fold and check); ``seat`` the hero; ``stacks`` / ``dealer`` the real hand's ((0, 0) = STACK);
    ``board_mode`` 0: the reference's bucket at an action node (every board card the hand carries), 1: the board at the node.
    Nothing is checked here: a malformed hand is answered with its status."""

    def __init__(self, holes, draws=(), plays=(), seat=0, stacks=(0, 0), dealer=0, board_mode=0):
        self.holes, self.draws, self.plays = tuple(holes), tuple(draws), tuple(plays)
        self.seat, self.stacks, self.dealer, self.board_mode = seat, tuple(stacks), dealer, board_mode

    @staticmethod
    def pack(hands) -> np.ndarray:
        """-> AIVAT_DTYPE[n]; plays past the cap keep their first 48 and their true number clipped to 255 (status LENGTH)"""
        if isinstance(hands, np.ndarray) and hands.dtype == AIVAT_DTYPE:
            return np.ascontiguousarray(hands)
        if isinstance(hands, AivatHand):
            hands = [hands]
        out = np.zeros(len(hands), AIVAT_DTYPE)
        for i, h in enumerate(hands):
            out[i]["hole"] = h.holes
            out[i]["draws"][: len(h.draws)] = h.draws
            out[i]["stacks"] = h.stacks
            out[i]["seat"], out[i]["dealer"], out[i]["board_mode"], out[i]["n_plays"] = h.seat, h.dealer, h.board_mode, min(len(h.plays), 255)
            for j, (kind, chips) in enumerate(h.plays[:MAX_PLAYS]):
                out[i]["kind"][j] = _lib.PLAY[kind] if isinstance(kind, str) else kind
                out[i]["chips"][j] = chips
        return out


class Frontier:
    """A depth-limited leaf (``DepthSampler::payoffs``, crates/nlhe/src/solver.rs:51-66): ``holes`` the two-card masks of seat 0 and
    seat 1; ``internal`` the seat whose utility is reported; ``draws`` / ``edges`` / ``stacks`` / ``dealer`` as in ``Recall`` — the
    history from ``Game::from_start`` to the frontier state; ``prefix``: the solver's construction prefix (edge codes), the start of
    every rollout's story, independent of ``edges``.  Nothing is checked here: a malformed frontier is answered with its status."""

    def __init__(self, holes, internal=0, draws=(), edges=(), prefix=(), stacks=(0, 0), dealer=0):
        self.holes, self.internal, self.draws, self.edges = tuple(holes), internal, tuple(draws), tuple(edges)
        self.prefix, self.stacks, self.dealer = tuple(prefix), tuple(stacks), dealer

    @staticmethod
    def pack(frontiers) -> np.ndarray:
        """-> FRONTIER_DTYPE[n]; edges / prefix longer than their caps keep their first entries and their true length clipped to 255
        (status LENGTH)"""
        if isinstance(frontiers, np.ndarray) and frontiers.dtype == FRONTIER_DTYPE:
            return np.ascontiguousarray(frontiers)
        if isinstance(frontiers, Frontier):
            frontiers = [frontiers]
        out = np.zeros(len(frontiers), FRONTIER_DTYPE)
        for i, f in enumerate(frontiers):
            out[i]["holes"] = f.holes
            out[i]["draws"][: len(f.draws)] = f.draws
            out[i]["stacks"] = f.stacks
            out[i]["internal"], out[i]["dealer"] = f.internal, f.dealer
            out[i]["n_edges"], out[i]["n_prefix"] = min(len(f.edges), 255), min(len(f.prefix), 255)
            k, m = min(len(f.edges), MAX_HISTORY), min(len(f.prefix), MAX_PREFIX)
            out[i]["edges"][:k] = f.edges[:k]
            out[i]["prefix"][:m] = f.prefix[:m]
        return out


class NlheSolver:
    """``mccfr!(Nlhe, NlheEncoder, NlheTurn, NlheEdge, NlheGame, NlheInfo, 128)`` (crates/nlhe/src/solver.rs:11) on one
    MI355X: ``step`` = ``Solver::step``, ``batch`` = ``Solver::batch`` (inspection), ``export`` / ``load`` = the blueprint
    rows by NlheInfo.  ``tables``: the encoder's four ``deuce.Lookup`` (pref, flop, turn, river); None = hash encoder.
    ``sampling``: "external" (the macro's default), "prunable", "pluribus" (the Flagship type)."""

    def __init__(self, cap_log2=20, regret="linear", weight="linear", batch=128, seed=0, hyper=None, tables=None, device=0,
                 sampling="external"):
        self._lib = _lib.load()
        self.hp = hyper
        if self.hp is None:
            self.hp = _lib.Hyper()
            self._lib.rp_hyper_default(C.byref(self.hp))
        self.batch_size = batch
        self.device = device
        self._tables = tables
        tab = None
        if tables is not None:
            arr = (C.c_void_p * 4)(*[t._h for t in tables])
            tab = C.cast(arr, C.c_void_p)
            self._tab_arr = arr
        self._h = C.c_void_p()
        _lib.check(self._lib.rp_nlhe_create(device, cap_log2, _lib.REGRET[regret], _lib.WEIGHT[weight], C.byref(self.hp), seed, batch,
                                            tab, C.byref(self._h)))
        if sampling != "external":  # Flagship = Nlhe<LinearRegret, LinearWeight, PluribusSampling> (nlhe/src/lib.rs:86-90)
            _lib.check(self._lib.rp_nlhe_set_sampling(self._h, _lib.SAMPLING[sampling]))

    def set_rng(self, kind: str):
        """"counter" (default) or "reference": opponent draws and Pluribus' coin from the reference's DefaultHasher -> SmallRng chain"""
        _lib.check(self._lib.rp_nlhe_set_rng(self._h, _lib.RNG[kind]))

    def set_exact(self, on: bool = True):
        """regret vectors in the reference's own float order on the batch-wide kernels too (always so up to 2 048 trees per step)"""
        _lib.check(self._lib.rp_nlhe_set_exact(self._h, 1 if on else 0))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rp_nlhe_destroy(self._h)
            self._h = None

    __del__ = close

    def step(self, mode="ordered"):
        _lib.check(self._lib.rp_nlhe_step(self._h, _lib.UPDATE[mode]))

    def train(self, mode="composed", max_steps=0, max_seconds=0.0, log_interval=60.0, flush_interval=1800.0, on_checkpoint=None,
              on_flush=None, interrupt=None):
        """``Trainer::train`` (crates/forge/src/trainer.rs:18-66) over this solver; returns Progress::summary"""
        return _lib.train(self._lib.rp_nlhe_train, self._h, _lib.UPDATE[mode], max_steps=max_steps, max_seconds=max_seconds,
                          log_interval=log_interval, flush_interval=flush_interval, on_checkpoint=on_checkpoint, on_flush=on_flush,
                          interrupt=interrupt)

    def profile(self, enable: bool):
        _lib.check(self._lib.rp_nlhe_profile(self._h, 1 if enable else 0))

    def kernel_times(self):
        """{group: (total_ms, launches)} since profile(True); groups: expand, children, sweeps, decide, apply"""
        return {name: _lib.kernel_time(self._lib.rp_nlhe_kernel_time, self._h, name)
                for name in ("expand", "children", "sweeps", "decide", "apply")}

    def census(self):
        """nodes of the profiled steps by kind + children of their walker nodes"""
        k, w = (C.c_uint64 * 4)(), C.c_uint64()
        _lib.check(self._lib.rp_nlhe_census(self._h, k, C.byref(w)))
        return dict(terminal=k[0], chance=k[1], walker=k[2], opponent=k[3], walker_children=w.value)

    def last_shape(self):
        """(levels, nodes) of the last traversed batch"""
        a, b = C.c_uint32(), C.c_uint32()
        _lib.check(self._lib.rp_nlhe_last_shape(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def batch(self, cap=1 << 22):
        n = C.c_uint32()
        _lib.check(self._lib.rp_nlhe_batch(self._h, 0, C.byref(n), *([None] * 9)))
        m = min(cap, n.value)
        out = dict(n=n.value, tree=np.zeros(m, np.uint32), past=np.zeros(m, np.uint64), present=np.zeros(m, np.uint32),
                   choices=np.zeros(m, np.uint64), n_actions=np.zeros(m, np.uint8), expanded=np.zeros(m, np.uint16),
                   regret=np.zeros((m, A), np.float32), policy=np.zeros((m, A), np.float32), payoff=np.zeros(m, np.float32))
        _lib.check(self._lib.rp_nlhe_batch(self._h, m, C.byref(n), _p(out["tree"]), _p(out["past"]), _p(out["present"]), _p(out["choices"]),
                                           _p(out["n_actions"]), _p(out["expanded"]), _p(out["regret"]), _p(out["policy"]), _p(out["payoff"])))
        return out

    # ---- multi-GPU exchange by infoset key (include/rp_mi355x.h rp_nlhe_step_local / step_apply) ----
    def set_shard(self, rank: int, world: int):
        _lib.check(self._lib.rp_nlhe_set_shard(self._h, rank, world))

    def entry_bytes(self):
        b, m = C.c_size_t(), C.c_uint32()
        _lib.check(self._lib.rp_nlhe_entry_bytes(self._h, C.byref(b), C.byref(m)))
        return b.value, m.value

    def step_local(self, entries_ptr: int, past_ptr: int, present_ptr: int, choices_ptr: int) -> int:
        n = C.c_uint32()
        _lib.check(self._lib.rp_nlhe_step_local(self._h, C.c_void_p(entries_ptr), C.c_void_p(past_ptr), C.c_void_p(present_ptr),
                                                C.c_void_p(choices_ptr), C.byref(n)))
        return n.value

    def step_apply(self, entries_ptr: int, past_ptr: int, present_ptr: int, choices_ptr: int, n: int):
        _lib.check(self._lib.rp_nlhe_step_apply(self._h, C.c_void_p(entries_ptr), C.c_void_p(past_ptr), C.c_void_p(present_ptr),
                                                C.c_void_p(choices_ptr), n))

    def step_comm(self, comm, steps: int = 1):
        """`steps` sharded steps over the library's own RCCL communicator (robopoker_amd.mccfr.Comm)"""
        _lib.check(self._lib.rp_nlhe_step_comm(self._h, comm.handle, steps))

    def set_stream(self, hip_stream_ptr):
        _lib.check(self._lib.rp_nlhe_set_stream(self._h, C.c_void_p(hip_stream_ptr)))

    def sync(self):
        _lib.check(self._lib.rp_nlhe_sync(self._h))

    @property
    def epoch(self) -> int:
        e = C.c_uint64()
        _lib.check(self._lib.rp_nlhe_epoch(self._h, C.byref(e)))
        return e.value

    def counters(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _lib.check(self._lib.rp_nlhe_counters(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def export(self):
        n = C.c_uint64()
        _lib.check(self._lib.rp_nlhe_export(self._h, 0, C.byref(n), None, None, None, None))
        m = n.value
        past, present, choices = np.zeros(m, np.uint64), np.zeros(m, np.uint32), np.zeros(m, np.uint64)
        enc = np.zeros((m, A), dtype=ENC_DTYPE)
        _lib.check(self._lib.rp_nlhe_export(self._h, m, C.byref(n), _p(past), _p(present), _p(choices), _p(enc)))
        return past, present, choices, enc

    def load(self, past, present, choices, enc, epoch: int):
        past, present, choices = (np.ascontiguousarray(past, np.uint64), np.ascontiguousarray(present, np.uint32),
                                  np.ascontiguousarray(choices, np.uint64))
        enc = np.ascontiguousarray(enc, dtype=ENC_DTYPE)
        _lib.check(self._lib.rp_nlhe_import(self._h, past.size, _p(past), _p(present), _p(choices), _p(enc), epoch))

    # ---- the table itself on the device (include/rp_mi355x.h THE TABLE ITSELF ON THE DEVICE) ----
    def capacity(self):
        """(cap_log2, infosets in the table)"""
        c, k = C.c_uint32(), C.c_uint64()
        _lib.check(self._lib.rp_nlhe_capacity(self._h, C.byref(c), C.byref(k)))
        return c.value, k.value

    def resize(self, cap_log2: int):
        """continue on a table of 2^cap_log2 slots, every infoset rehashed on the device (both tables resident during the call)"""
        _lib.check(self._lib.rp_nlhe_resize(self._h, int(cap_log2)))

    def set_growth(self, max_cap_log2: int, headroom: int = 0):
        """``step`` / ``train`` / ``load_device`` double the table up to 2^max_cap_log2 while 2 * (keys + headroom) > slots; 0 = off"""
        _lib.check(self._lib.rp_nlhe_set_growth(self._h, int(max_cap_log2), int(headroom)))

    def export_device(self, cap=None):
        """``export`` into torch tensors on the solver's device, in the same (slot) order: (past int64[m], present int32[m],
        choices int64[m], enc uint8[m,9,16], n) — torch spells u64 / u32 as int64 / int32; ``enc.cpu().numpy().view(ENC_DTYPE)[..., 0]``.
        n = the infosets in the table, m = min(cap, n) (cap None: all).  Synchronises the solver's stream."""
        d = torch.device(f"cuda:{self.device}")
        m = self.capacity()[1] if cap is None else min(int(cap), self.capacity()[1])
        past, present, choices = (torch.empty(m, dtype=torch.int64, device=d), torch.empty(m, dtype=torch.int32, device=d),
                                  torch.empty(m, dtype=torch.int64, device=d))
        enc = torch.empty((m, A, ENC_DTYPE.itemsize), dtype=torch.uint8, device=d)
        n = C.c_uint64()
        torch.cuda.current_stream(d).synchronize()
        _lib.check(self._lib.rp_nlhe_export_device(self._h, m, C.byref(n), _dptr(past, m), _dptr(present, m), _dptr(choices, m), _dptr(enc, m)))
        return past, present, choices, enc, n.value

    def load_device(self, past, present, choices, enc, epoch: int):
        """``load`` from device tensors (``export_device``'s): keys found or inserted and rows written on the device; a key named more
        than once keeps its last Encounters; sets the epoch.  Synchronises the solver's stream."""
        dev, past, present, choices = self._keys(past, present, choices)
        assert dev and isinstance(enc, torch.Tensor), "load_device takes device tensors (host arrays: load)"
        enc = enc.contiguous()
        n = past.numel()
        assert enc.is_cuda and enc.element_size() * enc.numel() == n * A * ENC_DTYPE.itemsize
        torch.cuda.current_stream(past.device).synchronize()
        _lib.check(self._lib.rp_nlhe_import_device(self._h, n, _dptr(past, n), _dptr(present, n), _dptr(choices, n), _dptr(enc, n), int(epoch)))

    # ---- the read side: what the blueprint says about infosets given BY KEY (include/rp_mi355x.h rp_nlhe_policy / rp_nlhe_memory) ----
    def _keys(self, past, present, choices):
        """-> (on_device, past, present, choices): torch device tensors go to the _device forms, anything else through numpy to the host forms"""
        if isinstance(past, torch.Tensor):
            ks = [t.contiguous() for t in (past, present, choices)]
            assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in ks), "keys: three device tensors or three host arrays"
            assert ks[0].element_size() == 8 and ks[1].element_size() == 4 and ks[2].element_size() == 8  # torch spells u64 / u32 as int64 / int32
            assert ks[0].numel() == ks[1].numel() == ks[2].numel()
            return True, *ks
        ks = (np.ascontiguousarray(past, np.uint64), np.ascontiguousarray(present, np.uint32), np.ascontiguousarray(choices, np.uint64))
        assert ks[0].size == ks[1].size == ks[2].size
        return False, *ks

    def _queue(self, fn, d, live, keys, *args):
        """a _device call on the solver's stream: whatever produced the inputs on torch's current stream has finished first; tensors
        among ``args`` go as addresses (``_dptr``); ``keys``, which the queued launch reads, stay referenced"""
        torch.cuda.current_stream(d).synchronize()
        _lib.check(fn(self._h, *[_dptr(a, live) if isinstance(a, torch.Tensor) else a for a in args]))
        self._query_keys = keys

    def policy(self, past, present, choices, kind="averaged"):
        """``Brain::policy`` / ``Source::strategy`` for n infosets: dict(policy float32[n,9], edges uint8[n,9], n_actions uint8[n],
        found bool[n]); kind: "iterated", "averaged", "sampling".  Read-only.  Device tensors in -> device tensors out, queued on the
        solver's stream (``sync()`` waits); numpy in -> numpy out."""
        dev, past, present, choices = self._keys(past, present, choices)
        if dev:
            n, d = past.numel(), past.device
            out = dict(policy=torch.empty((n, A), dtype=torch.float32, device=d), edges=torch.empty((n, A), dtype=torch.uint8, device=d),
                       n_actions=torch.empty(n, dtype=torch.uint8, device=d), found=torch.empty(n, dtype=torch.uint8, device=d))
            self._queue(self._lib.rp_nlhe_policy_device, d, n, (past, present, choices), _lib.DIST[kind], n, past, present, choices,
                        out["policy"], out["edges"], out["n_actions"], out["found"])
            out["found"] = out["found"].view(torch.bool)
            return out
        n = past.size
        out = dict(policy=np.zeros((n, A), np.float32), edges=np.zeros((n, A), np.uint8), n_actions=np.zeros(n, np.uint8),
                   found=np.zeros(n, np.uint8))
        _lib.check(self._lib.rp_nlhe_policy(self._h, _lib.DIST[kind], n, _p(past), _p(present), _p(choices), _p(out["policy"]),
                                            _p(out["edges"]), _p(out["n_actions"]), _p(out["found"])))
        out["found"] = out["found"].view(np.bool_)
        return out

    def memory(self, past, present, choices):
        """``Source::memory`` for n infosets: (enc ENC_DTYPE[n,9], n_actions uint8[n], found bool[n]).  Device tensors in -> enc is a device
        tensor uint8[n,9,16] (``.cpu().numpy().view(ENC_DTYPE)[..., 0]``), queued on the solver's stream."""
        dev, past, present, choices = self._keys(past, present, choices)
        if dev:
            n, d = past.numel(), past.device
            enc = torch.empty((n, A, ENC_DTYPE.itemsize), dtype=torch.uint8, device=d)
            nact, found = torch.empty(n, dtype=torch.uint8, device=d), torch.empty(n, dtype=torch.uint8, device=d)
            self._queue(self._lib.rp_nlhe_memory_device, d, n, (past, present, choices), n, past, present, choices, enc, nact, found)
            return enc, nact, found.view(torch.bool)
        n = past.size
        enc, nact, found = np.zeros((n, A), dtype=ENC_DTYPE), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        _lib.check(self._lib.rp_nlhe_memory(self._h, n, _p(past), _p(present), _p(choices), _p(enc), _p(nact), _p(found)))
        return enc, nact, found.view(np.bool_)

    # ---- the blueprint census (include/rp_mi355x.h rp_nlhe_table_census): what the table says as a whole ----
    def table_census(self):
        """one read-only scan of the table -> the rp_census record as a CENSUS_DTYPE scalar array (shape ()): cell[5][32], infosets[5],
        epoch, slots, cold / hot lists.  ``census_stats`` / ``census_street_stats`` / ``census_saturation`` / ``census_grid_usage`` /
        ``census_cold`` / ``census_hot`` read it.  (``census()`` is the profiled steps' node census.)"""
        rec = np.zeros((), CENSUS_DTYPE)
        _lib.check(self._lib.rp_nlhe_table_census(self._h, _p(rec)))
        return rec

    def table_census_device(self, out=None):
        """the same record as a device tensor uint8[20800], queued on the solver's stream (``sync()`` waits;
        ``.cpu().numpy().view(CENSUS_DTYPE)[0]``).  ``out``: a tensor to reuse."""
        if out is None:
            out = torch.empty(CENSUS_DTYPE.itemsize, dtype=torch.uint8, device=f"cuda:{self.device}")
        assert out.is_cuda and out.is_contiguous() and out.element_size() * out.numel() == CENSUS_DTYPE.itemsize
        self._queue(self._lib.rp_nlhe_table_census_device, out.device, True, None, out)
        return out

    # ---- ranges (include/rp_mi355x.h rp_nlhe_reaches / rp_nlhe_opponent_range): the blueprint's reach of every hole a seat could hold ----
    def reaches_raw(self, recalls, kind="opponent", normalize=False):
        """the untrimmed arrays of rp_nlhe_reaches: dict(count uint32[n], holes uint64[n,1326], reach float32[n,1326], status uint8[n])"""
        rec = Recall.pack(recalls)
        n = rec.size
        out = dict(count=np.zeros(n, np.uint32), holes=np.zeros((n, MAX_HOLES), np.uint64), reach=np.zeros((n, MAX_HOLES), np.float32),
                   status=np.zeros(n, np.uint8))
        _lib.check(self._lib.rp_nlhe_reaches(self._h, _lib.REACH[kind], 1 if normalize else 0, n, _p(rec), _p(out["count"]), _p(out["holes"]),
                                             _p(out["reach"]), _p(out["status"])))
        return out

    def reaches(self, recalls, kind="opponent", normalize=False):
        """``opponent_reaches`` / ``signalled_reaches`` (nlhe/src/solver.rs:162-169,227-240) for n recalls: a list of
        (holes uint64[count], reach float32[count], status) in ``HandIterator`` order; status != 0 (malformed recall): empty arrays."""
        raw = self.reaches_raw(recalls, kind, normalize)
        return [(raw["holes"][i, :c].copy(), raw["reach"][i, :c].copy(), int(raw["status"][i])) for i, c in enumerate(raw["count"])]

    def opponent_observations(self, recalls):
        """``Nlhe::opponent_observations`` (solver.rs:206-208): the villain's holes with reaches normalised to sum to 1"""
        return self.reaches(recalls, "opponent", True)

    def signalled_observations(self, recalls):
        """``Nlhe::signalled_observations`` (solver.rs:221-223): what hero's own line says about hero's hole"""
        return self.reaches(recalls, "signalled", True)

    def opponent_range(self, recalls):
        """``Nlhe::opponent_range`` (solver.rs:192-197), the Posterior over abstraction buckets of the board's street:
        (mass float32[n,256], seen bool[n,256], status uint8[n])"""
        rec = Recall.pack(recalls)
        n = rec.size
        mass, seen, status = np.zeros((n, BUCKETS), np.float32), np.zeros((n, BUCKETS), np.uint8), np.zeros(n, np.uint8)
        _lib.check(self._lib.rp_nlhe_opponent_range(self._h, n, _p(rec), _p(mass), _p(seen), _p(status)))
        return mass, seen.view(np.bool_), status

    def reaches_device(self, recalls_dev, kind="opponent", normalize=False):
        """rp_nlhe_reaches_device: ``recalls_dev`` a device uint8 tensor [n, 88] (``torch.from_numpy(Recall.pack(..).view(np.uint8))``);
        -> dict of device tensors (count int32[n], holes int64[n,1326], reach float32[n,1326], status uint8[n]), queued on the
        solver's stream (``sync()`` waits)"""
        rec, n, d = _records(recalls_dev, RECALL_DTYPE)
        out = dict(count=torch.empty(n, dtype=torch.int32, device=d), holes=torch.empty((n, MAX_HOLES), dtype=torch.int64, device=d),
                   reach=torch.empty((n, MAX_HOLES), dtype=torch.float32, device=d), status=torch.empty(n, dtype=torch.uint8, device=d))
        self._queue(self._lib.rp_nlhe_reaches_device, d, n, (rec,), _lib.REACH[kind], 1 if normalize else 0, n, rec, out["count"], out["holes"],
                    out["reach"], out["status"])
        return out

    def opponent_range_device(self, recalls_dev):
        """rp_nlhe_opponent_range_device: -> device tensors (mass float32[n,256], seen uint8[n,256], status uint8[n])"""
        rec, n, d = _records(recalls_dev, RECALL_DTYPE)
        mass = torch.empty((n, BUCKETS), dtype=torch.float32, device=d)
        seen, status = torch.empty((n, BUCKETS), dtype=torch.uint8, device=d), torch.empty(n, dtype=torch.uint8, device=d)
        self._queue(self._lib.rp_nlhe_opponent_range_device, d, n, (rec,), n, rec, mass, seen, status)
        return mass, seen, status

    # ---- AIVAT (include/rp_mi355x.h rp_nlhe_aivat): the blueprint's control variates of played hands ----
    def aivat(self, hands):
        """``Aivat::corrections`` (crates/arena/src/aivat.rs:63-145) for n hands: dict(hero, villain, chance, total float32[n],
        n_action, n_chance, status uint8[n]); ``won + total`` is the hand's adjusted value.  Read-only."""
        hd = AivatHand.pack(hands)
        n = hd.size
        out = {k: np.zeros(n, np.float32) for k in ("hero", "villain", "chance", "total")}
        out.update({k: np.zeros(n, np.uint8) for k in ("n_action", "n_chance", "status")})
        _lib.check(self._lib.rp_nlhe_aivat(self._h, n, _p(hd), *[_p(out[k]) for k in ("hero", "villain", "chance", "total", "n_action",
                                                                                    "n_chance", "status")]))
        return out

    def aivat_device(self, hands_dev):
        """rp_nlhe_aivat_device: ``hands_dev`` a device uint8 tensor [n, 192] (``torch.from_numpy(AivatHand.pack(..).view(np.uint8))``);
        -> the same dict of device tensors, queued on the solver's stream (``sync()`` waits)"""
        hd, n, d = _records(hands_dev, AIVAT_DTYPE)
        out = {k: torch.empty(n, dtype=torch.float32, device=d) for k in ("hero", "villain", "chance", "total")}
        out.update({k: torch.empty(n, dtype=torch.uint8, device=d) for k in ("n_action", "n_chance", "status")})
        self._queue(self._lib.rp_nlhe_aivat_device, d, n, (hd,), n, hd, *[out[k] for k in ("hero", "villain", "chance", "total", "n_action",
                                                                                          "n_chance", "status")])
        return out

    @staticmethod
    def aivat_summarize(adjusted, raw_stddev):
        """``Aivat::summarize`` (aivat.rs:45-61) over the adjusted values of a match: dict(won, mean, stderr, reduction, pvalue) as
        float32; ``raw_stddev``: the standard deviation of the raw winnings.  Host arithmetic, no device."""
        x = np.ascontiguousarray(adjusted, np.float32).ravel()
        s = _lib.AivatSummary()
        _lib.check(_lib.load().rp_aivat_summarize(x.size, _p(x), float(raw_stddev), C.byref(s)))
        return {k: np.float32(getattr(s, k)) for k in ("won", "mean", "stderr", "reduction", "pvalue")}

    # ---- matches (include/rp_mi355x.h rp_nlhe_match): hands played on the device between two agents, as AIVAT's records ----
    @staticmethod
    def _match_args(seed=0, first_id=0, stacks=(0, 0), agents=("blueprint", "blueprint"), dealer=2, hero=0, mirror=False, snap=False,
                    board_mode=1):
        """rp_nlhe_match_args; ``agents``: "blueprint" / "dirac" / "fish" (or rp_agent_kind codes) of seat 0 and seat 1"""
        a = _lib.NlheMatchArgs()
        _lib.load().rp_nlhe_match_args_default(C.byref(a))
        a.seed, a.first_id, a.dealer, a.hero, a.mirror, a.snap, a.board_mode = seed, first_id, dealer, hero, int(mirror), int(snap), board_mode
        a.stacks[0], a.stacks[1] = stacks
        a.agent[0], a.agent[1] = (_lib.AGENT[k] if isinstance(k, str) else k for k in agents)
        return a

    def match(self, n, opponent=None, **args):
        """n heads-up hands between seat 0 reading this solver's table and seat 1 reading ``opponent``'s (None: this one), the table of
        ``parlor/src/engine.rs`` seating ``Agent<Blueprint>`` / ``Dirac`` / ``Fish``: dict(hands AIVAT_DTYPE[n], the records
        ``aivat`` takes as they are; won int16[n], the hero's chips; rejected uint8[n]; status uint8[n]).  ``args``: seed, first_id,
        stacks, agents, dealer (2 = alternating), hero, mirror, snap, board_mode.  Hand i draws from the counter streams of
        ``first_id + i``: a batch split into calls with matching ``first_id`` answers the same bytes.  Read-only on both tables."""
        a, n = self._match_args(**args), int(n)
        out = dict(hands=np.zeros(n, AIVAT_DTYPE), won=np.zeros(n, np.int16), rejected=np.zeros(n, np.uint8), status=np.zeros(n, np.uint8))
        _lib.check(self._lib.rp_nlhe_match(self._h, opponent._h if opponent is not None else None, n, C.byref(a), _p(out["hands"]),
                                           _p(out["won"]), _p(out["rejected"]), _p(out["status"])))
        return out

    def match_device(self, n, opponent=None, **args):
        """rp_nlhe_match_device: -> the same dict of device tensors (hands uint8[n, 192], which ``aivat_device`` takes as it is), queued
        on the solver's stream after what ``opponent``'s stream holds (``sync()`` waits)"""
        a, n, d = self._match_args(**args), int(n), torch.device("cuda", self.device)
        out = dict(hands=torch.empty((n, AIVAT_DTYPE.itemsize), dtype=torch.uint8, device=d), won=torch.empty(n, dtype=torch.int16, device=d),
                   rejected=torch.empty(n, dtype=torch.uint8, device=d), status=torch.empty(n, dtype=torch.uint8, device=d))
        _lib.check(self._lib.rp_nlhe_match_device(self._h, opponent._h if opponent is not None else None, n, C.byref(a),
                                                  *[_dptr(out[k], n) for k in ("hands", "won", "rejected", "status")]))
        return out

    # ---- translation (include/rp_mi355x.h rp_nlhe_translate): played hands to the recalls the ranges, beliefs and re-solves read ----
    @staticmethod
    def _translate_args(kind="snap", seed=0, first_id=0):
        """rp_nlhe_translate_args; ``kind``: "snap" / "harmonic" / "phargmax" (or an rp_translation_kind code)"""
        a = _lib.NlheTranslateArgs()
        _lib.load().rp_nlhe_translate_args_default(C.byref(a))
        a.seed, a.first_id, a.kind = seed, first_id, _lib.TRANSLATE[kind] if isinstance(kind, str) else kind
        return a

    def translate(self, hands, kind="snap", pov=None, upto=None, seed=0, first_id=0):
        """``Recall::history()`` under ``Translation::Snap`` / ``Harmonic`` / ``Phargmax`` for n played hands (``AivatHand``s, or the
        records ``match`` writes): dict(recalls RECALL_DTYPE[n], the records ``reaches`` and ``belief`` take, seen from seat ``pov[i]``
        (None: the hand's ``seat``) after the first ``upto[i]`` plays (None: all); play_edges uint8[n,48], the edge of each play;
        past uint64[n], present uint32[n], choices uint64[n], the key of the recall's head as ``policy`` takes it; n_choices uint8[n];
        status uint8[n]).  Harmonic draws for hand i from the counter stream of ``first_id + i``.  Read-only."""
        hd = AivatHand.pack(hands)
        n = hd.size
        pov = None if pov is None else np.ascontiguousarray(pov, np.uint8)
        upto = None if upto is None else np.ascontiguousarray(upto, np.uint8)
        assert (pov is None or pov.size == n) and (upto is None or upto.size == n)
        out = dict(recalls=np.zeros(n, RECALL_DTYPE), play_edges=np.zeros((n, MAX_PLAYS), np.uint8), past=np.zeros(n, np.uint64),
                   present=np.zeros(n, np.uint32), choices=np.zeros(n, np.uint64), n_choices=np.zeros(n, np.uint8), status=np.zeros(n, np.uint8))
        _lib.check(self._lib.rp_nlhe_translate(self._h, n, C.byref(self._translate_args(kind, seed, first_id)), _p(hd), _p(pov), _p(upto),
                                               *[_p(out[k]) for k in ("recalls", "play_edges", "past", "present", "choices", "n_choices",
                                                                      "status")]))
        return out

    def translate_device(self, hands_dev, kind="snap", pov=None, upto=None, seed=0, first_id=0):
        """rp_nlhe_translate_device: ``hands_dev`` a device uint8 tensor [n, 192] (``match_device``'s ``hands``), ``pov`` / ``upto`` device
        uint8 tensors [n] or None; -> the same dict of device tensors (recalls uint8[n, 88], which ``reaches_device`` and
        ``belief_device`` take as it is; past / choices int64[n], present int32[n], which ``policy`` takes), queued on the solver's
        stream (``sync()`` waits)"""
        hd, n, d = _records(hands_dev, AIVAT_DTYPE)
        pov, upto = (None if t is None else t.contiguous() for t in (pov, upto))
        assert all(t is None or (t.is_cuda and t.element_size() == 1 and t.numel() == n) for t in (pov, upto))
        out = dict(recalls=torch.empty((n, RECALL_DTYPE.itemsize), dtype=torch.uint8, device=d),
                   play_edges=torch.empty((n, MAX_PLAYS), dtype=torch.uint8, device=d), past=torch.empty(n, dtype=torch.int64, device=d),
                   present=torch.empty(n, dtype=torch.int32, device=d), choices=torch.empty(n, dtype=torch.int64, device=d),
                   n_choices=torch.empty(n, dtype=torch.uint8, device=d), status=torch.empty(n, dtype=torch.uint8, device=d))
        self._queue(self._lib.rp_nlhe_translate_device, d, n, (hd, pov, upto), n, C.byref(self._translate_args(kind, seed, first_id)), hd,
                    pov, upto, *[out[k] for k in ("recalls", "play_edges", "past", "present", "choices", "n_choices", "status")])
        return out

    # ---- search matches (include/rp_mi355x.h rp_nlhe_search_match): a seat may re-solve every postflop decision ----
    @staticmethod
    def _search_args(search=("none", "none"), origin_mode=0, iterations=None, rollouts=None, bias=None, prior=None, visit_threshold=None,
                     steps_cap=0, search_seed=0, **match):
        """rp_nlhe_search_args; ``search``: "none" / "world" (or rp_search_kind codes) of seat 0 and seat 1; the library's defaults where
        an argument is None; everything else is ``_match_args``'s"""
        a = _lib.NlheSearchArgs()
        _lib.load().rp_nlhe_search_args_default(C.byref(a))
        a.match = NlheSolver._match_args(**match)
        a.search[0], a.search[1] = (_lib.SEARCH[k] if isinstance(k, str) else k for k in search)
        a.origin_mode, a.steps_cap, a.search_seed = int(origin_mode), int(steps_cap), search_seed
        for k, v in (("iterations", iterations), ("rollouts", rollouts), ("visit_threshold", visit_threshold)):
            if v is not None:
                setattr(a, k, int(v))
        for k, v in (("bias", bias), ("prior", prior)):
            if v is not None:
                setattr(a, k, v)
        return a

    def search_match(self, n, opponent=None, **args):
        """``match`` in which a seat may be a search agent (``Agent<World<Blueprint>>``, with "dirac" its Dirac form): at every postflop
        decision the seat builds the opponent's range from its own table (``belief``), re-solves the rest of the street
        (``subgame_solve`` with ``iterations``, ``rollouts``, ``bias``, ``prior``, ``search_seed`` and the id ``hand_id * 256 + decision``)
        and plays the blend of the harvest and its blueprint by visit counts (``visit_threshold``).  ``args``: ``match``'s, plus search,
        origin_mode (0: no frontier; 1: the entry street - 1), steps_cap (traced decisions per hand).  -> ``match``'s dict plus
        searched uint8[n], unsolved uint8[n] (search decisions that fell back to the blueprint) and steps
        SEARCH_STEP_DTYPE[n, steps_cap].  Read-only on both tables."""
        a, n = self._search_args(**args), int(n)
        out = dict(hands=np.zeros(n, AIVAT_DTYPE), won=np.zeros(n, np.int16), rejected=np.zeros(n, np.uint8), status=np.zeros(n, np.uint8),
                   searched=np.zeros(n, np.uint8), unsolved=np.zeros(n, np.uint8))
        steps = np.zeros((max(n, 1), a.steps_cap), SEARCH_STEP_DTYPE)  # a trace is asked for with an address, even for an empty batch
        _lib.check(self._lib.rp_nlhe_search_match(self._h, opponent._h if opponent is not None else None, n, C.byref(a),
                                                  *[_p(out[k]) for k in ("hands", "won", "rejected", "status", "searched", "unsolved")],
                                                  _p(steps) if a.steps_cap else None))
        out["steps"] = steps[:n]
        return out

    def search_match_device(self, n, opponent=None, **args):
        """rp_nlhe_search_match_device: -> the same dict of device tensors (hands uint8[n, 192], steps uint8[n, steps_cap, 352]).  Unlike
        ``match_device`` the call returns when the match is finished: it waits on the solver's stream once per round of solves"""
        a, n, d = self._search_args(**args), int(n), torch.device("cuda", self.device)
        out = dict(hands=torch.empty((n, AIVAT_DTYPE.itemsize), dtype=torch.uint8, device=d), won=torch.empty(n, dtype=torch.int16, device=d))
        out.update({k: torch.empty(n, dtype=torch.uint8, device=d) for k in ("rejected", "status", "searched", "unsolved")})
        steps = torch.empty((max(n, 1), a.steps_cap, SEARCH_STEP_DTYPE.itemsize), dtype=torch.uint8, device=d)  # an address even for n = 0
        _lib.check(self._lib.rp_nlhe_search_match_device(self._h, opponent._h if opponent is not None else None, n, C.byref(a),
                                                         *[_dptr(out[k], n) for k in ("hands", "won", "rejected", "status", "searched", "unsolved")],
                                                         _dptr(steps, a.steps_cap)))
        out["steps"] = steps[:n]
        return out

    @staticmethod
    def match_summary(won):
        """the bb/100 statistics of ``spar/src/benchmark.rs`` over the winnings of a match in chips: dict(hands, total_bb, bb_per_100,
        stddev, confidence) as float64 (hands: int).  Host arithmetic, no device."""
        x = np.ascontiguousarray(won, np.int16).ravel()
        s = _lib.MatchSummary()
        _lib.check(_lib.load().rp_match_summarize(x.size, _p(x), C.byref(s)))
        return dict(hands=int(s.hands), **{k: np.float64(getattr(s, k)) for k in ("total_bb", "bb_per_100", "stddev", "confidence")})

    # ---- frontier payoffs (include/rp_mi355x.h rp_nlhe_frontier_payoffs): biased continuation rollouts from depth-limited leaves ----
    def frontier_payoffs(self, frontiers, bias=5.0, rollouts=16, seed=0, first_id=0, return_won=False):
        """``DepthSampler::payoffs`` for n frontiers: (payoffs float32[n,4,4], status uint8[n]), payoffs[i,k,j] = the mean utility of
        seat ``internal`` when it continues with strategy k and the other seat with j (0 blueprint, 1 fold-, 2 call-, 3 raise-biased).
        ``return_won``: also won int16[n,16,rollouts], every rollout's utility.  Rollout r of cell (k, j) of frontier i draws from
        the counter stream ((first_id + i) * 16 + 4 k + j) * rollouts + r of ``seed``: a batch split into calls with matching
        ``first_id`` answers the same bits.  Read-only."""
        fr = Frontier.pack(frontiers)
        n, r = fr.size, max(int(rollouts), 1)
        pay, status = np.zeros((n, LEAVES, LEAVES), np.float32), np.zeros(n, np.uint8)
        won = np.zeros((n, LEAVES * LEAVES, min(r, MAX_ROLLOUTS)), np.int16) if return_won else None
        _lib.check(self._lib.rp_nlhe_frontier_payoffs(self._h, n, _p(fr), bias, int(rollouts), seed, first_id, _p(pay), _p(won), _p(status)))
        return (pay, status, won) if return_won else (pay, status)

    def frontier_payoffs_device(self, frontiers_dev, bias=5.0, rollouts=16, seed=0, first_id=0, return_won=False):
        """rp_nlhe_frontier_payoffs_device: ``frontiers_dev`` a device uint8 tensor [n, 112]
        (``torch.from_numpy(Frontier.pack(..).view(np.uint8))``); -> device tensors (payoffs float32[n,4,4], status uint8[n]) and, with
        ``return_won``, won int16[n,16,rollouts], queued on the solver's stream (``sync()`` waits)"""
        (fr, n, d), r = _records(frontiers_dev, FRONTIER_DTYPE), max(int(rollouts), 1)
        pay = torch.empty((n, LEAVES, LEAVES), dtype=torch.float32, device=d)
        status = torch.empty(n, dtype=torch.uint8, device=d)
        won = torch.empty((n, LEAVES * LEAVES, min(r, MAX_ROLLOUTS)), dtype=torch.int16, device=d) if return_won else None
        self._queue(self._lib.rp_nlhe_frontier_payoffs_device, d, n, (fr,), n, fr, bias, int(rollouts), seed, first_id, pay, won, status)
        return (pay, status, won) if return_won else (pay, status)

    # ---- depth-limited re-solve (include/rp_mi355x.h rp_nlhe_depth_solve): DepthSolver steps and harvest, many solves per launch ----
    @staticmethod
    def _solve_args(struct, default_fn, iterations, rollouts, bias, prior, seed, first_id, rows_cap, deals_cap=None):
        """rp_nlhe_depth_args / rp_nlhe_subgame_args (``deals_cap``): the library's defaults where an argument is None"""
        a = struct()
        default_fn(C.byref(a))
        a.iterations, a.seed, a.first_id, a.rows_cap = int(iterations), seed, first_id, int(rows_cap)
        if deals_cap is not None:
            a.deals_cap = int(deals_cap)
        if rollouts is not None:
            a.rollouts = int(rollouts)
        if bias is not None:
            a.bias = bias
        if prior is not None:
            a.prior = prior
        return a

    @staticmethod
    def depth_entries(entries) -> np.ndarray:
        """-> FRONTIER_DTYPE[n]; an entry given as a ``Frontier`` without a prefix gets the reference's (``subgame_descents``: the
        trailing choice edges of its history)"""
        if isinstance(entries, Frontier):
            entries = [entries]
        if isinstance(entries, (list, tuple)):
            filled = []
            for f in entries:
                if not f.prefix:
                    tail = []
                    for e in reversed(f.edges):
                        if e == 1:  # Draw
                            break
                        tail.append(e)
                    f = Frontier(f.holes, f.internal, f.draws, f.edges, tail[::-1], f.stacks, f.dealer)
                filled.append(f)
            entries = filled
        return Frontier.pack(entries)

    @staticmethod
    def _origin(origin, n, none_value=ORIGIN_ENTRY):
        """-> int8[n] or None; ``none_value``: what a None among per-entry origins reads as (ORIGIN_ENTRY: depth, ORIGIN_NONE: subgame)"""
        if origin is None:
            return None
        o = np.full(n, origin, np.int8) if np.isscalar(origin) else np.array([none_value if x is None else x for x in origin], np.int8)
        assert o.size == n
        return o

    def depth_solve(self, entries, origin=None, iterations=1, rollouts=None, bias=None, prior=None, seed=0, first_id=0, rows_cap=0):
        """``DepthSolver`` for n entries (``Frontier`` records: ``internal`` the seat solved for, ``edges`` the history to the entry
        state, ``prefix`` the construction prefix, derived where empty): ``iterations`` steps each, then the ``Harvest`` at the entry
        state.  ``origin``: None = every entry's own street, which is ``adapt_leaf`` as written (chance leaves valued by stored
        payoffs, no rollouts); an int or one per entry (None = that entry's street) = the depth beyond which a chance node is a
        frontier, ``street - 1`` for the 4 x 4 continuation game at the next street boundary.  -> (results DEPTH_RESULT_DTYPE[n],
        rows DEPTH_ROW_DTYPE[n, rows_cap]): ``refined`` the iterated distribution over the entry infoset's choices, ``rows`` the
        solve's local profile sorted by (kind, past, present, choices).  Solve i draws from the streams of ``first_id + i`` under
        ``seed``: a batch split into calls with matching ``first_id`` answers the same bits.  Read-only."""
        en = self.depth_entries(entries)
        n = en.size
        a = self._solve_args(_lib.NlheDepthArgs, self._lib.rp_nlhe_depth_args_default, iterations, rollouts, bias, prior, seed, first_id, rows_cap)
        o = self._origin(origin, n)
        res, rows = np.zeros(n, DEPTH_RESULT_DTYPE), np.zeros((n, int(rows_cap)), DEPTH_ROW_DTYPE)
        _lib.check(self._lib.rp_nlhe_depth_solve(self._h, n, _p(en), _p(o), C.byref(a), _p(res), _p(rows) if rows_cap else None))
        return res, rows

    def depth_solve_device(self, entries_dev, origin_dev=None, iterations=1, rollouts=None, bias=None, prior=None, seed=0, first_id=0,
                           rows_cap=0):
        """rp_nlhe_depth_solve_device: ``entries_dev`` a device uint8 tensor [n, 112], ``origin_dev`` a device int8 tensor [n] or None;
        -> device uint8 tensors (results [n, 144], rows [n, rows_cap, 168]) queued on the solver's stream (``sync()`` waits); view
        them with DEPTH_RESULT_DTYPE / DEPTH_ROW_DTYPE on the host"""
        en, n, d = _records(entries_dev, FRONTIER_DTYPE)
        assert origin_dev is None or (origin_dev.is_cuda and origin_dev.dtype == torch.int8 and origin_dev.numel() == n)
        a = self._solve_args(_lib.NlheDepthArgs, self._lib.rp_nlhe_depth_args_default, iterations, rollouts, bias, prior, seed, first_id, rows_cap)
        res = torch.empty((n, DEPTH_RESULT_DTYPE.itemsize), dtype=torch.uint8, device=d)
        rows = torch.empty((n, int(rows_cap), DEPTH_ROW_DTYPE.itemsize), dtype=torch.uint8, device=d)
        self._queue(self._lib.rp_nlhe_depth_solve_device, d, n, (en, origin_dev), n, en, origin_dev, C.byref(a), res,
                    rows if int(rows_cap) else None)
        return res, rows

    # ---- safe subgame re-solve (include/rp_mi355x.h rp_nlhe_subgame_solve): SubGameSolver steps and harvest, many solves per launch ----
    @staticmethod
    def subgame_recalls(entries) -> np.ndarray:
        """-> RECALL_DTYPE[n]: the recall whose belief a subgame solve of each entry wants — ``internal``'s point of view of the
        entry's history (``belief(subgame_recalls(entries))`` yields ``hole_world`` / ``weights`` for ``subgame_solve``)"""
        en = NlheSolver.depth_entries(entries)
        rec = np.zeros(en.size, RECALL_DTYPE)
        for i, f in enumerate(en):
            rec[i]["hole"] = f["holes"][min(int(f["internal"]), 1)]
            for k in ("draws", "stacks", "dealer", "n_edges", "edges"):
                rec[i][k] = f[k]
            rec[i]["pov"] = f["internal"]
        return rec

    def subgame_solve(self, entries, beliefs, origin=None, iterations=1, rollouts=None, bias=None, prior=None, seed=0, first_id=0, rows_cap=0,
                      deals_cap=0):
        """``SubGameSolver`` (``adapt_full``; ``adapt_safe`` answers the same) for n entries as ``depth_solve`` takes them, except that
        the hole of the seat opposite ``internal`` is not read: before every iteration that seat is dealt a hole from a world drawn
        from the belief (``NlheEncoder::restrict``, deal ``t`` of ``restrict(.., deals=4096)`` for the same ``seed`` / ``first_id``),
        and every infoset of that iteration's tree is tagged with the world.  ``beliefs``: (hole_world uint8[n,1326], weights
        float32[n,4]) or the dict ``belief()`` returns.  ``origin``: None (or None per entry) = no frontier, the solver as written — the
        tree is the rest of the entry street, chance leaves valued by stored payoffs; an int in -1 .. 3 = ``with_origin``.
        -> (results SUBGAME_RESULT_DTYPE[n], rows SUBGAME_ROW_DTYPE[n, rows_cap] sorted by (world, kind, past, present, choices),
        deals SUBGAME_DEAL_DTYPE[n, deals_cap]): ``refined`` averages the four worlds' iterated distributions.  Read-only."""
        en = self.depth_entries(entries)
        n = en.size
        if isinstance(beliefs, dict):
            beliefs = (beliefs["hole_world"], beliefs["weights"])
        hw = np.ascontiguousarray(beliefs[0], np.uint8).reshape(n, MAX_HOLES)
        wt = np.ascontiguousarray(beliefs[1], np.float32).reshape(n, WORLDS)
        a = self._solve_args(_lib.NlheSubgameArgs, self._lib.rp_nlhe_subgame_args_default, iterations, rollouts, bias, prior, seed, first_id,
                             rows_cap, deals_cap)
        o = self._origin(origin, n, ORIGIN_NONE)
        res, rows = np.zeros(n, SUBGAME_RESULT_DTYPE), np.zeros((n, int(rows_cap)), SUBGAME_ROW_DTYPE)
        deals = np.zeros((n, int(deals_cap)), SUBGAME_DEAL_DTYPE)
        _lib.check(self._lib.rp_nlhe_subgame_solve(self._h, n, _p(en), _p(hw), _p(wt), _p(o), C.byref(a), _p(res), _p(rows) if rows_cap else None,
                                                   _p(deals) if deals_cap else None))
        return res, rows, deals

    def subgame_solve_device(self, entries_dev, hole_world_dev, weights_dev, origin_dev=None, iterations=1, rollouts=None, bias=None, prior=None,
                             seed=0, first_id=0, rows_cap=0, deals_cap=0):
        """rp_nlhe_subgame_solve_device: ``entries_dev`` a device uint8 tensor [n, 112]; ``hole_world_dev`` uint8 [n, 1326] and
        ``weights_dev`` float32 [n, 4] as ``belief_device`` returns them (no host copy in between); ``origin_dev`` a device int8
        tensor [n] or None; -> device uint8 tensors (results [n, 176], rows [n, rows_cap, 168], deals [n, deals_cap, 16]) queued on the
        solver's stream (``sync()`` waits); view them with the SUBGAME_*_DTYPEs on the host"""
        (en, n, d), hw, wt = _records(entries_dev, FRONTIER_DTYPE), hole_world_dev.contiguous(), weights_dev.contiguous()
        assert hw.is_cuda and hw.element_size() == 1 and hw.numel() == n * MAX_HOLES
        assert wt.is_cuda and wt.dtype == torch.float32 and wt.numel() == n * WORLDS
        assert origin_dev is None or (origin_dev.is_cuda and origin_dev.dtype == torch.int8 and origin_dev.numel() == n)
        a = self._solve_args(_lib.NlheSubgameArgs, self._lib.rp_nlhe_subgame_args_default, iterations, rollouts, bias, prior, seed, first_id,
                             rows_cap, deals_cap)
        res = torch.empty((n, SUBGAME_RESULT_DTYPE.itemsize), dtype=torch.uint8, device=d)
        rows = torch.empty((n, int(rows_cap), SUBGAME_ROW_DTYPE.itemsize), dtype=torch.uint8, device=d)
        deals = torch.empty((n, int(deals_cap), SUBGAME_DEAL_DTYPE.itemsize), dtype=torch.uint8, device=d)
        self._queue(self._lib.rp_nlhe_subgame_solve_device, d, n, (en, hw, wt, origin_dev), n, en, hw, wt, origin_dev, C.byref(a), res,
                    rows if int(rows_cap) else None, deals if int(deals_cap) else None)
        return res, rows, deals

    # ---- subgame worlds (include/rp_mi355x.h rp_nlhe_partition / rp_nlhe_belief / rp_nlhe_restrict): the opponent's range in quantile worlds ----
    def partition(self, mass, seen):
        """``Posterior::partition::<4>`` for n rows of (mass float32[n,256], seen bool[n,256]), as ``opponent_range`` returns them:
        (world uint8[n,256], weights float32[n,4]); world 0 holds the buckets of highest mass, WORLD_NONE marks a bucket that is no entry"""
        mass = np.ascontiguousarray(mass, np.float32).reshape(-1, BUCKETS)
        seen = np.ascontiguousarray(np.asarray(seen) != 0, np.uint8).reshape(-1, BUCKETS)
        n = mass.shape[0]
        assert seen.shape[0] == n
        world, weights = np.zeros((n, BUCKETS), np.uint8), np.zeros((n, WORLDS), np.float32)
        _lib.check(self._lib.rp_nlhe_partition(self._h, n, _p(mass), _p(seen), _p(world), _p(weights)))
        return world, weights

    def partition_device(self, mass_dev, seen_dev):
        """rp_nlhe_partition_device: device tensors (mass float32[n,256], seen uint8[n,256]), as ``opponent_range_device`` returns them ->
        device tensors (world uint8[n,256], weights float32[n,4]), queued on the solver's stream (``sync()`` waits)"""
        mass, seen = mass_dev.contiguous(), seen_dev.contiguous()
        assert mass.is_cuda and seen.is_cuda and mass.dtype == torch.float32 and seen.element_size() == 1
        assert mass.numel() % BUCKETS == 0 and seen.numel() == mass.numel()
        n, d = mass.numel() // BUCKETS, mass.device
        world, weights = torch.empty((n, BUCKETS), dtype=torch.uint8, device=d), torch.empty((n, WORLDS), dtype=torch.float32, device=d)
        self._queue(self._lib.rp_nlhe_partition_device, d, n, (mass, seen), n, mass, seen, world, weights)
        return world, weights

    def belief(self, recalls):
        """``Nlhe::setup`` (solver.rs:129-136) = ``opponent_range(recall).partition()`` for n recalls: dict(world uint8[n,256],
        weights float32[n,4], hole_world uint8[n,1326] — the world of every candidate hole in ``HandIterator`` order, WORLD_NONE past
        the recall's count — and status uint8[n])"""
        rec = Recall.pack(recalls)
        n = rec.size
        out = dict(world=np.zeros((n, BUCKETS), np.uint8), weights=np.zeros((n, WORLDS), np.float32),
                   hole_world=np.zeros((n, MAX_HOLES), np.uint8), status=np.zeros(n, np.uint8))
        _lib.check(self._lib.rp_nlhe_belief(self._h, n, _p(rec), _p(out["world"]), _p(out["weights"]), _p(out["hole_world"]), _p(out["status"])))
        return out

    def belief_device(self, recalls_dev):
        """rp_nlhe_belief_device: ``recalls_dev`` as for ``reaches_device`` -> dict of device tensors as ``belief`` returns them"""
        rec, n, d = _records(recalls_dev, RECALL_DTYPE)
        out = dict(world=torch.empty((n, BUCKETS), dtype=torch.uint8, device=d), weights=torch.empty((n, WORLDS), dtype=torch.float32, device=d),
                   hole_world=torch.empty((n, MAX_HOLES), dtype=torch.uint8, device=d), status=torch.empty(n, dtype=torch.uint8, device=d))
        self._queue(self._lib.rp_nlhe_belief_device, d, n, (rec,), n, rec, out["world"], out["weights"], out["hole_world"], out["status"])
        return out

    def restrict(self, recalls, deals=1, worlds=None, seed=0, first_id=0):
        """``NlheEncoder::restrict`` for n recalls, ``deals`` opponent holes each: dict(holes uint64[n,deals], world uint8[n,deals] — the
        world asked for or drawn — attempts uint16[n,deals] (MAX_REJECTIONS: the unconstrained fallback) and status uint8[n]).
        ``worlds``: None (every world is drawn from the belief's weights) or uint8[n,deals] of 0..3 / WORLD_NONE (draw).  Deal d of
        recall r draws from the counter stream (first_id + r) * deals + d of ``seed`` (epoch 1): a batch split into calls with
        matching ``first_id`` answers the same holes.  Read-only."""
        rec = Recall.pack(recalls)
        n, deals = rec.size, int(deals)
        w = None if worlds is None else np.ascontiguousarray(worlds, np.uint8).reshape(n, deals)
        out = dict(holes=np.zeros((n, deals), np.uint64), world=np.zeros((n, deals), np.uint8), attempts=np.zeros((n, deals), np.uint16),
                   status=np.zeros(n, np.uint8))
        _lib.check(self._lib.rp_nlhe_restrict(self._h, n, _p(rec), deals, _p(w), seed, first_id, _p(out["holes"]), _p(out["world"]),
                                              _p(out["attempts"]), _p(out["status"])))
        return out

    def restrict_device(self, recalls_dev, deals=1, worlds_dev=None, seed=0, first_id=0):
        """rp_nlhe_restrict_device: ``recalls_dev`` as for ``reaches_device``, ``worlds_dev`` None or a device uint8 tensor [n, deals] ->
        dict of device tensors (holes int64[n,deals], world uint8[n,deals], attempts int16[n,deals], status uint8[n]), queued on the
        solver's stream (``sync()`` waits)"""
        (rec, n, d), deals = _records(recalls_dev, RECALL_DTYPE), int(deals)
        w = None
        if worlds_dev is not None:
            w = worlds_dev.contiguous()
            assert w.is_cuda and w.element_size() == 1 and w.numel() == n * deals
        out = dict(holes=torch.empty((n, deals), dtype=torch.int64, device=d), world=torch.empty((n, deals), dtype=torch.uint8, device=d),
                   attempts=torch.empty((n, deals), dtype=torch.int16, device=d), status=torch.empty(n, dtype=torch.uint8, device=d))
        self._queue(self._lib.rp_nlhe_restrict_device, d, n and deals, (rec, w), n, rec, deals, w, seed, first_id, out["holes"], out["world"],
                    out["attempts"], out["status"])
        return out


def playouts(n_players: int, n_games: int, seed: int, max_steps: int = 200, device: int = 0):
    """-> (payoffs float32[n_games][n_players], digests int64[n_games] (the u64 bit patterns), steps int32[n_games])."""
    dev = torch.device("cuda", device)
    pay = torch.empty((n_games, n_players), dtype=torch.float32, device=dev)
    dig = torch.empty(n_games, dtype=torch.int64, device=dev)
    steps = torch.empty(n_games, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    _lib.check(_lib.load().rp_nlhe_playouts(device, n_players, n_games, seed, max_steps, pay.data_ptr(), dig.data_ptr(), steps.data_ptr()))
    return pay, dig, steps

"""ctypes binding of librp_mi355x.so (include/rp_mi355x.h).

This is the Python face of the C-ABI: plain pointers and sizes, no torch types.  The library is
built in-tree by ``__graft_entry__.build()`` (``make -C robopoker_amd/csrc``); importing this module
when the shared object is missing raises — there is no CPU fallback for the product path.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librp_mi355x.so")

RP_OK = 0
RP_ERR_INVALID = 1
RP_ERR_NO_DEVICE = 2
RP_ERR_HIP = 3
RP_ERR_UNSUPPORTED = 4
RP_ERR_CAPACITY = 5

RP_TURN_CHANCE = 254
RP_TURN_TERMINAL = 255
RP_NO_INFO = 0xFFFFFFFF

# enums (rp_regret_kind, rp_weight_kind, rp_sampling_kind, rp_game_kind, rp_dist_kind, rp_metric_kind)
REGRET = {"summed": 0, "linear": 1, "discounted": 2, "floored": 3, "asymmetric": 4}
WEIGHT = {"constant": 0, "linear": 1, "quadratic": 2, "exponential": 3}
SAMPLING = {"external": 0, "prunable": 1, "pluribus": 2}
GAME = {"kuhn": 0, "leduc": 1, "rps": 2, "leduc_wide": 3}
DIST = {"iterated": 0, "averaged": 1, "sampling": 2}
METRIC = {"sinkhorn": 0, "variation": 1}
UPDATE = {"ordered": 0, "composed": 1}
REACH = {"opponent": 0, "signalled": 1}  # rp_reach_kind
RP_NLHE_MAX_HISTORY = 48
RP_NLHE_MAX_HOLES = 1326
RP_NLHE_FRONTIER_LEAVES = 4
RP_NLHE_MAX_PREFIX = 12
RP_NLHE_WORLDS = 4
RP_NLHE_MAX_REJECTIONS = 10000
RP_WORLD_NONE = 0xFF
RP_NLHE_DEPTH_MAX_ITERATIONS = 4096
RP_NLHE_DEPTH_MAX_FRONTIERS = 32
RP_NLHE_DEPTH_MAX_NODES = 384
RP_NLHE_DEPTH_MAX_ROWS = 512
RP_NLHE_DEPTH_ORIGIN_ENTRY = 127
RP_DEPTH_NODES, RP_DEPTH_ROWS, RP_DEPTH_FRONTIERS = 8, 9, 10
RP_NLHE_SUBGAME_MAX_ROWS = 2048
RP_NLHE_SUBGAME_ORIGIN_NONE = 126
RP_MCCFR_SUBGAME_MAX_ITERATIONS = 1 << 20
RP_MCCFR_SUBGAME_MAX_NODES, RP_MCCFR_SUBGAME_MAX_ROWS, RP_MCCFR_SUBGAME_MAX_INFOS, RP_MCCFR_SUBGAME_MAX_CANDIDATES = 62, 1024, 8192, 16
(RP_MSUB_OK, RP_MSUB_SEAT, RP_MSUB_MODE, RP_MSUB_WORLDS, RP_MSUB_COUNT, RP_MSUB_STATE, RP_MSUB_SECRET, RP_MSUB_PATH, RP_MSUB_WEIGHT, RP_MSUB_INFO,
 RP_MSUB_TREE, RP_MSUB_ROWS, RP_MSUB_ORDER, RP_MSUB_FRONTIER) = range(14)
RP_MCCFR_ORIGIN_ENTRY, RP_MCCFR_ORIGIN_NONE = 254, 255
RP_AIVAT_MAX_PLAYS = 48
RP_AIVAT_WITNESS = 11
PLAY = {"fold": 1, "call": 2, "check": 3, "raise": 4, "shove": 5}  # rp_aivat_play
AGENT = {"blueprint": 0, "dirac": 1, "fish": 2}  # rp_agent_kind
SEARCH = {"none": 0, "world": 1}  # rp_search_kind
TRANSLATE = {"snap": 0, "harmonic": 1, "phargmax": 2}  # rp_translation_kind
RP_NLHE_SEARCH_MAX_SOLVES = 48


class Hyper(C.Structure):
    _fields_ = [
        ("temperature", C.c_float),
        ("smoothing", C.c_float),
        ("curiosity", C.c_float),
        ("prune_threshold", C.c_float),
        ("prune_explore", C.c_float),
        ("prune_warmup", C.c_uint64),
        ("regret_min", C.c_float),
        ("_pad", C.c_uint32),
    ]


class Encounter(C.Structure):
    _fields_ = [("weight", C.c_float), ("regret", C.c_float), ("payoff", C.c_float), ("visits", C.c_uint32)]


class MccfrSubgameArgs(C.Structure):  # rp_mccfr_subgame_args, 32 bytes
    _fields_ = [("iterations", C.c_uint32), ("prior", C.c_float), ("seed", C.c_uint64), ("first_id", C.c_uint64), ("rows_cap", C.c_uint32),
                ("reserved", C.c_uint32)]


class MccfrFrontiers(C.Structure):  # rp_mccfr_frontiers: host arrays, copied by rp_mccfr_set_frontiers
    _fields_ = [("depth", C.c_void_p), ("pick_info", C.c_void_p), ("payoff_ref", C.c_void_p), ("matrices", C.c_void_p), ("n_pick", C.c_uint32),
                ("n_matrices", C.c_uint32), ("leaves", C.c_uint32), ("reserved", C.c_uint32)]


class NlheRecall(C.Structure):
    """rp_nlhe_recall: what one seat has seen, at edge level (88 bytes)"""
    _fields_ = [("hole", C.c_uint64), ("draws", C.c_uint64 * 3), ("stacks", C.c_int16 * 2), ("pov", C.c_uint8), ("dealer", C.c_uint8),
                ("n_edges", C.c_uint8), ("reserved", C.c_uint8), ("edges", C.c_uint8 * 48)]


class AivatHand(C.Structure):
    """rp_aivat_hand: one played heads-up hand, action level (192 bytes)"""
    _fields_ = [("hole", C.c_uint64 * 2), ("draws", C.c_uint64 * 3), ("stacks", C.c_int16 * 2), ("chips", C.c_int16 * 48),
                ("kind", C.c_uint8 * 48), ("seat", C.c_uint8), ("dealer", C.c_uint8), ("n_plays", C.c_uint8), ("board_mode", C.c_uint8)]


class AivatSummary(C.Structure):
    """rp_aivat_summary: Aivat::summarize's figures"""
    _fields_ = [("won", C.c_float), ("mean", C.c_float), ("stderr", C.c_float), ("reduction", C.c_float), ("pvalue", C.c_float)]


class NlheMatchArgs(C.Structure):
    """rp_nlhe_match_args: one per call (32 bytes)"""
    _fields_ = [("seed", C.c_uint64), ("first_id", C.c_uint64), ("stacks", C.c_int16 * 2), ("agent", C.c_uint8 * 2), ("dealer", C.c_uint8),
                ("hero", C.c_uint8), ("mirror", C.c_uint8), ("snap", C.c_uint8), ("board_mode", C.c_uint8), ("reserved", C.c_uint8 * 5)]


class NlheTranslateArgs(C.Structure):
    """rp_nlhe_translate_args: one per call (24 bytes)"""
    _fields_ = [("seed", C.c_uint64), ("first_id", C.c_uint64), ("kind", C.c_uint8), ("reserved", C.c_uint8 * 7)]


class NlheSearchArgs(C.Structure):
    """rp_nlhe_search_args: one per call (72 bytes)"""
    _fields_ = [("match", NlheMatchArgs), ("search_seed", C.c_uint64), ("iterations", C.c_uint32), ("rollouts", C.c_uint32), ("bias", C.c_float),
                ("prior", C.c_float), ("visit_threshold", C.c_uint32), ("steps_cap", C.c_uint32), ("search", C.c_uint8 * 2),
                ("origin_mode", C.c_uint8), ("reserved0", C.c_uint8 * 5)]


class MatchSummary(C.Structure):
    """rp_match_summary: the bb/100 figures of a series of winnings (40 bytes)"""
    _fields_ = [("hands", C.c_uint64), ("total_bb", C.c_double), ("bb_per_100", C.c_double), ("stddev", C.c_double), ("confidence", C.c_double)]


RP_NLHE_CENSUS_TOP, RP_NLHE_CENSUS_SEGMENT, RP_NLHE_CENSUS_STREETS, RP_NLHE_CENSUS_CODES = 64, 65536, 5, 32


class CensusCell(C.Structure):
    """rp_census_cell: one (street, edge code) cell of the blueprint census (104 bytes)"""
    _fields_ = [("rows", C.c_uint64), ("rated", C.c_uint64), ("dominant", C.c_uint64), ("visits", C.c_uint64),
                ("ratio", C.c_double), ("weight", C.c_double), ("total", C.c_double), ("regret", C.c_double), ("payoff", C.c_double),
                ("max_regret", C.c_float), ("min_regret", C.c_float), ("max_weight", C.c_float), ("max_payoff", C.c_float),
                ("min_payoff", C.c_float), ("max_visits", C.c_uint32), ("min_visits", C.c_uint32), ("reserved", C.c_uint32)]


class CensusEntry(C.Structure):
    """rp_census_entry: one infoset of a ranked list (32 bytes)"""
    _fields_ = [("past", C.c_uint64), ("choices", C.c_uint64), ("present", C.c_uint32), ("edges", C.c_uint32),
                ("visits", C.c_uint32), ("regret", C.c_float)]


class Census(C.Structure):
    """rp_census: the record of one scan of the blueprint table (20 800 bytes)"""
    _fields_ = [("cell", CensusCell * 32 * 5), ("infosets", C.c_uint64 * 5), ("epoch", C.c_uint64), ("slots", C.c_uint64),
                ("n_cold", C.c_uint32), ("n_hot", C.c_uint32), ("cold", CensusEntry * 64), ("hot", CensusEntry * 64)]


class CensusTotals(C.Structure):
    """rp_census_totals: ApiBlueprintStats (64 bytes)"""
    _fields_ = [("infosets", C.c_uint64), ("edges", C.c_uint64), ("avg_regret", C.c_float), ("max_regret", C.c_float),
                ("min_regret", C.c_float), ("avg_weight", C.c_float), ("max_weight", C.c_float), ("avg_payoff", C.c_float),
                ("max_payoff", C.c_float), ("min_payoff", C.c_float), ("avg_visits", C.c_float), ("max_visits", C.c_uint32),
                ("min_visits", C.c_uint32), ("reserved", C.c_uint32)]


class CensusStreet(C.Structure):
    """rp_census_street: ApiStreetStats (40 bytes)"""
    _fields_ = [("infosets", C.c_uint64), ("edges", C.c_uint64), ("avg_regret", C.c_float), ("avg_weight", C.c_float),
                ("avg_payoff", C.c_float), ("avg_visits", C.c_float), ("street", C.c_char), ("reserved", C.c_uint8 * 7)]


class CensusPeaks(C.Structure):
    """rp_census_peaks: ApiSaturation (32 bytes)"""
    _fields_ = [("max_weight", C.c_float), ("max_regret", C.c_float), ("max_payoff", C.c_float), ("max_visits", C.c_uint32),
                ("precision_f32", C.c_float), ("weight_pct", C.c_float), ("regret_pct", C.c_float), ("reserved", C.c_uint32)]


class CensusGrid(C.Structure):
    """rp_census_grid: ApiGridUsage (32 bytes)"""
    _fields_ = [("n_decisions_with_edge", C.c_uint64), ("n_dominant", C.c_uint64), ("avg_freq", C.c_float), ("weighted_freq", C.c_float),
                ("street", C.c_uint8), ("edge", C.c_uint8), ("reserved", C.c_uint8 * 6)]


class NlheFrontier(C.Structure):
    """rp_nlhe_frontier: a depth-limited leaf — both holes, the history to it and the solver's prefix (112 bytes)"""
    _fields_ = [("holes", C.c_uint64 * 2), ("draws", C.c_uint64 * 3), ("stacks", C.c_int16 * 2), ("internal", C.c_uint8),
                ("dealer", C.c_uint8), ("n_edges", C.c_uint8), ("n_prefix", C.c_uint8), ("edges", C.c_uint8 * 48),
                ("prefix", C.c_uint8 * 12), ("reserved", C.c_uint8 * 4)]


class NlheDepthArgs(C.Structure):
    """rp_nlhe_depth_args: one per call (40 bytes)"""
    _fields_ = [("iterations", C.c_uint32), ("rollouts", C.c_uint32), ("bias", C.c_float), ("prior", C.c_float), ("seed", C.c_uint64),
                ("first_id", C.c_uint64), ("rows_cap", C.c_uint32), ("reserved", C.c_uint32)]


class NlheDepthResult(C.Structure):
    """rp_nlhe_depth_result: the Harvest of one solve and its counters (144 bytes)"""
    _fields_ = [("past", C.c_uint64), ("choices", C.c_uint64), ("present", C.c_uint32), ("n_actions", C.c_uint8), ("status", C.c_uint8),
                ("pad", C.c_uint8 * 2), ("refined", C.c_float * 9), ("visits", C.c_uint32 * 9), ("regret", C.c_float),
                ("sum_regret", C.c_float), ("iterations", C.c_uint32), ("n_rows", C.c_uint32), ("nodes", C.c_uint64),
                ("infosets", C.c_uint64), ("frontiers", C.c_uint64), ("rollouts", C.c_uint64)]


class NlheSubgameArgs(C.Structure):
    """rp_nlhe_subgame_args: one per call (48 bytes)"""
    _fields_ = [("iterations", C.c_uint32), ("rollouts", C.c_uint32), ("bias", C.c_float), ("prior", C.c_float), ("seed", C.c_uint64),
                ("first_id", C.c_uint64), ("rows_cap", C.c_uint32), ("deals_cap", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class NlheSubgameResult(C.Structure):
    """rp_nlhe_subgame_result: the Harvest of one solve over the four worlds, its counters and its deals' (176 bytes)"""
    _fields_ = NlheDepthResult._fields_ + [("drawn", C.c_uint32 * 4), ("attempts", C.c_uint64), ("fallbacks", C.c_uint32), ("pad2", C.c_uint32)]


class NlheSearchStep(C.Structure):
    """rp_nlhe_search_step: one traced search decision of a search match (352 bytes)"""
    _fields_ = [("solve_id", C.c_uint64), ("recall", NlheRecall), ("result", NlheSubgameResult), ("bp", C.c_float * 9), ("p", C.c_float * 9),
                ("decision", C.c_uint32), ("seat", C.c_uint8), ("edge", C.c_uint8), ("fallback", C.c_uint8), ("belief_status", C.c_uint8)]


class NlheSubgameRow(C.Structure):
    """rp_nlhe_subgame_row: one row of a solve's world-tagged local profile (168 bytes)"""
    _fields_ = [("kind", C.c_uint8), ("n_actions", C.c_uint8), ("world", C.c_uint8), ("pad", C.c_uint8), ("present", C.c_uint32),
                ("past", C.c_uint64), ("choices", C.c_uint64), ("enc", Encounter * 9)]


class NlheSubgameDeal(C.Structure):
    """rp_nlhe_subgame_deal: the deal of one iteration (16 bytes)"""
    _fields_ = [("hole", C.c_uint64), ("world", C.c_uint8), ("pad", C.c_uint8), ("attempts", C.c_uint16), ("pad2", C.c_uint32)]


class NlheDepthRow(C.Structure):
    """rp_nlhe_depth_row: one row of a solve's local profile (168 bytes)"""
    _fields_ = [("kind", C.c_uint8), ("n_actions", C.c_uint8), ("pad", C.c_uint8 * 2), ("present", C.c_uint32), ("past", C.c_uint64),
                ("choices", C.c_uint64), ("enc", Encounter * 9)]


class State(C.Structure):
    _fields_ = [
        ("turn", C.c_uint8),
        ("n_children", C.c_uint8),
        ("chance_info", C.c_uint16),
        ("info", C.c_uint32),
        ("offset", C.c_uint32),
    ]


class HashStream(C.Structure):
    """rp_hash_stream: what `impl Hash for I` writes for one infoset (reference-seed mode)"""
    _fields_ = [("len", C.c_uint8), ("bytes", C.c_uint8 * 55)]


class HashStreams(C.Structure):
    _fields_ = [("n_infos", C.c_uint32), ("n_chance", C.c_uint32), ("infos", C.POINTER(HashStream)),
                ("chance", C.POINTER(HashStream))]


RNG = {"counter": 0, "reference": 1}


class GameTable(C.Structure):
    _fields_ = [
        ("n_states", C.c_uint32),
        ("n_infos", C.c_uint32),
        ("n_players", C.c_uint32),
        ("max_actions", C.c_uint32),
        ("n_children", C.c_uint32),
        ("n_terminals", C.c_uint32),
        ("train_root", C.c_uint32),
        ("exploit_root", C.c_uint32),
        ("max_depth", C.c_uint32),
        ("max_tree_nodes", C.c_uint32),
        ("states", C.POINTER(State)),
        ("children", C.POINTER(C.c_uint32)),
        ("payoffs", C.POINTER(C.c_float)),
        ("info_actions", C.POINTER(C.c_uint8)),
        ("info_player", C.POINTER(C.c_uint8)),
        ("default_regret", C.POINTER(C.c_float)),
    ]


class Decisions(C.Structure):
    """rp_decisions: one batch of Decisions in DEVICE memory (raw pointers)."""
    _fields_ = [
        ("n", C.c_uint32),
        ("row", C.c_void_p),
        ("n_actions", C.c_void_p),
        ("expanded", C.c_void_p),
        ("regret", C.c_void_p),
        ("policy", C.c_void_p),
        ("payoff", C.c_void_p),
    ]


class SinkhornHP(C.Structure):
    _fields_ = [("temperature", C.c_float), ("iterations", C.c_uint32), ("tolerance", C.c_float)]


class AtlasSample(C.Structure):  # rp_atlas_sample, 32 bytes
    _fields_ = [("obs", C.c_int64), ("equity", C.c_float), ("density", C.c_float), ("distance", C.c_float), ("position", C.c_uint32),
                ("population", C.c_uint32), ("abs", C.c_int16), ("reserved", C.c_uint8 * 2)]


ATLAS_STATUS = {"ok": 0, "miss": 1, "same": 2, "empty": 3, "range": 4}  # rp_atlas_status
ATLAS_HIST = {"abs": 0, "obs": 1}  # rp_atlas_hist_kind


class RpError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"rp_mi355x error {code}: {msg}")
        self.code = code


# every symbol include/rp_mi355x.h declares (tests/test_abi.py checks the list against the header)
class PruneStats(C.Structure):
    """rp_prune_stats (include/rp_mi355x.h): what the MFMA Sinkhorn bound discarded and what it cost"""
    _fields_ = [("enabled", C.c_uint32), ("reserved", C.c_uint32), ("points", C.c_uint64), ("candidates", C.c_uint64),
                ("survivors", C.c_uint64), ("block_iterations", C.c_uint64), ("cost_passes", C.c_uint64),
                ("mfma_instructions", C.c_uint64), ("audited_points", C.c_uint64), ("audit_mismatches", C.c_uint64),
                ("sampled_points", C.c_uint64), ("sample_mismatches", C.c_uint64), ("kpp_bound_pairs", C.c_uint64),
                ("kpp_bound_kept", C.c_uint64), ("kpp_bound_iterations", C.c_uint64), ("kpp_bound_cost_passes", C.c_uint64),
                ("column_iterations", C.c_uint64), ("ref_pick_chunks", C.c_uint64), ("ref_pick_walked", C.c_uint64)]


_SIGNATURES = {
    "rp_last_error": (C.c_char_p, []),
    "rp_device_count": (C.c_int, []),
    "rp_version": (C.c_char_p, []),
    "rp_math_selftest": (C.c_int, [C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rp_libm_glibc_sweep": (C.c_int, [C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]),
    "rp_libm_glibc_tab_sweep": (C.c_int, [C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]),
    "rp_math_exp_sweep": (C.c_int, [C.c_int, C.POINTER(C.c_uint64)]),
    "rp_sortscan_selftest": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32] + [C.c_void_p] * 8),
    "rp_hyper_default": (None, [C.POINTER(Hyper)]),
    "rp_game_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "rp_game_view": (C.c_int, [C.c_void_p, C.POINTER(GameTable)]),
    "rp_game_destroy": (C.c_int, [C.c_void_p]),
    "rp_game_info_id": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint32)]),
    "rp_game_info_name": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t]),
    "rp_game_table_check": (C.c_int, [C.POINTER(GameTable)]),
    "rp_mccfr_create": (
        C.c_int,
        [C.POINTER(GameTable), C.c_int, C.c_int, C.c_int, C.c_uint32, C.POINTER(Hyper), C.c_uint64, C.c_int,
         C.POINTER(C.c_void_p)],
    ),
    "rp_mccfr_create_mode": (
        C.c_int,
        [C.POINTER(GameTable), C.c_int, C.c_int, C.c_int, C.c_uint32, C.POINTER(Hyper), C.c_uint64, C.c_int, C.c_int,
         C.POINTER(C.c_void_p)],
    ),
    "rp_mccfr_destroy": (C.c_int, [C.c_void_p]),
    "rp_mccfr_step": (C.c_int, [C.c_void_p]),
    "rp_mccfr_solve": (C.c_int, [C.c_void_p, C.c_uint64]),
    "rp_mccfr_spend": (C.c_int, [C.c_void_p, C.c_double, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "rp_mccfr_step_async": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rp_mccfr_sync": (C.c_int, [C.c_void_p]),
    "rp_mccfr_epoch": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "rp_mccfr_counters": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "rp_mccfr_get": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(Encounter)]),
    "rp_mccfr_set": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(Encounter)]),
    "rp_mccfr_export": (C.c_int, [C.c_void_p, C.POINTER(Encounter), C.c_uint64]),
    "rp_mccfr_import": (C.c_int, [C.c_void_p, C.POINTER(Encounter), C.c_uint64, C.c_uint64]),
    "rp_mccfr_policy": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    "rp_mccfr_exploitability": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "rp_mccfr_exploitability_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rp_mccfr_best_response": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_float)]),
    "rp_mccfr_nash_variant": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "rp_mccfr_solve_to": (C.c_int, [C.c_void_p, C.c_float, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_float),
                                    C.POINTER(C.c_int)]),
    "rp_mccfr_sum_regret": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "rp_mccfr_subgame_args_default": (None, [C.POINTER(MccfrSubgameArgs)]),
    "rp_mccfr_subgame_belief": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rp_mccfr_subgame_belief_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rp_mccfr_subgame_solve": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(MccfrSubgameArgs), C.c_void_p, C.c_void_p]),
    "rp_mccfr_subgame_solve_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(MccfrSubgameArgs), C.c_void_p, C.c_void_p]),
    "rp_mccfr_set_frontiers": (C.c_int, [C.c_void_p, C.POINTER(MccfrFrontiers)]),
    "rp_game_frontiers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]),
    "rp_mccfr_depth_solve": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(MccfrSubgameArgs), C.c_void_p, C.c_void_p]),
    "rp_mccfr_depth_solve_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(MccfrSubgameArgs), C.c_void_p, C.c_void_p]),
    "rp_mccfr_set_batch": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rp_mccfr_set_update_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "rp_mccfr_set_rng": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(HashStreams)]),
    "rp_game_hash_streams": (C.c_int, [C.c_void_p, C.POINTER(HashStreams)]),
    "rp_mccfr_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rp_mccfr_traversal_variant": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "rp_mccfr_traversal_rows_bytes": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "rp_mccfr_fold_variant": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "rp_game_skeleton": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "rp_mccfr_set_shard": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "rp_mccfr_summary_bytes": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "rp_mccfr_step_local": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rp_mccfr_step_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "rp_mccfr_window_local": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "rp_mccfr_window_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "rp_comm_unique_id": (C.c_int, [C.c_void_p]),
    "rp_comm_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "rp_comm_adopt": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "rp_comm_destroy": (C.c_int, [C.c_void_p]),
    "rp_mccfr_step_comm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    "rp_kmeans_step_comm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "rp_mccfr_profile": (C.c_int, [C.c_void_p, C.c_int]),
    "rp_mccfr_kernel_time": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "rp_profile_create": (C.c_int, [C.c_int, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.POINTER(Hyper), C.c_void_p, C.c_uint32,
                                    C.POINTER(C.c_void_p)]),
    "rp_profile_destroy": (C.c_int, [C.c_void_p]),
    "rp_profile_apply": (C.c_int, [C.c_void_p, C.POINTER(Decisions), C.c_int]),
    "rp_profile_sync": (C.c_int, [C.c_void_p]),
    "rp_profile_epoch": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "rp_profile_set_epoch": (C.c_int, [C.c_void_p, C.c_uint64]),
    "rp_profile_get_rows": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "rp_profile_policy": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rp_profile_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rp_profile_entry_bytes": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "rp_profile_summarize": (C.c_int, [C.c_void_p, C.POINTER(Decisions), C.c_void_p, C.POINTER(C.c_uint32)]),
    "rp_profile_fold": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "rp_profile_profile": (C.c_int, [C.c_void_p, C.c_int]),
    "rp_profile_kernel_time": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "rp_sinkhorn_hp_default": (None, [C.POINTER(SinkhornHP)]),
    "rp_kmeans_create": (
        C.c_int,
        [C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(SinkhornHP), C.c_uint64,
         C.c_int, C.POINTER(C.c_void_p)],
    ),
    "rp_kmeans_create_device": (
        C.c_int,
        [C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(SinkhornHP), C.c_uint64,
         C.c_int, C.POINTER(C.c_void_p)],
    ),
    "rp_kmeans_destroy": (C.c_int, [C.c_void_p]),
    "rp_kmeans_init_centroids": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rp_kmeans_set_centroids": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rp_kmeans_set_centroid": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "rp_kmeans_get_point": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]),
    "rp_kmeans_kpp_begin": (C.c_int, [C.c_void_p]),
    "rp_kmeans_kpp_total": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "rp_kmeans_kpp_pick": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "rp_kmeans_kpp_update": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rp_kmeans_kpp_ref_walk": (C.c_int, [C.c_void_p, C.c_float, C.POINTER(C.c_float)]),
    "rp_kmeans_kpp_ref_draw": (C.c_int, [C.c_void_p, C.c_float, C.POINTER(C.c_float)]),
    "rp_kmeans_kpp_ref_pick": (C.c_int, [C.c_void_p, C.c_float, C.POINTER(C.c_uint64)]),
    "rp_kmeans_init_bounds": (C.c_int, [C.c_void_p]),
    "rp_kmeans_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "rp_kmeans_step_naive": (C.c_int, [C.c_void_p]),
    "rp_kmeans_assign": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rp_kmeans_bounds": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rp_kmeans_centroids": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rp_kmeans_metric": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rp_kmeans_rms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "rp_kmeans_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "rp_kmeans_exp_evals": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "rp_kmeans_prune_stats": (C.c_int, [C.c_void_p, C.POINTER(PruneStats)]),
    "rp_kmeans_bound_intervals": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rp_kmeans_kpp_bound_probe": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "rp_kmeans_kpp_bound_probe_at": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]),
    "rp_kmeans_refresh_stats": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rp_kmeans_upper_interval": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rp_kmeans_pairwise_last": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rp_weighted_index_probe": (C.c_int, [C.c_int, C.c_uint64, C.c_void_p, C.c_float, C.c_int, C.c_void_p]),
    "rp_weighted_index_probe_shards": (C.c_int, [C.c_int, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_float, C.c_void_p,
                                                  C.c_void_p]),
    "rp_kmeans_stats_ex": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rp_kmeans_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rp_kmeans_profile": (C.c_int, [C.c_void_p, C.c_int]),
    "rp_kmeans_kernel_time": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "rp_kmeans_partial_bytes": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "rp_kmeans_step_local": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rp_kmeans_step_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "rp_sinkhorn_set_libm": (C.c_int, [C.c_int]),
    "rp_sinkhorn_divergence": (
        C.c_int,
        [C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SinkhornHP), C.c_int, C.c_void_p],
    ),
    "rp_sinkhorn_cost": (
        C.c_int,
        [C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SinkhornHP), C.c_int, C.c_void_p,
         C.c_void_p],
    ),
    "rp_sinkhorn_cost_device": (
        C.c_int,
        [C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SinkhornHP), C.c_int, C.c_void_p,
         C.c_void_p],
    ),
    "rp_sinkhorn_flow": (C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SinkhornHP), C.c_int, C.c_void_p, C.c_void_p]),
    "rp_equity_variation": (C.c_int, [C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "rp_mccfr_train": (C.c_int, [C.c_void_p, C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                 C.POINTER(C.c_int), C.c_char_p, C.c_size_t]),
    "rp_nlhe_create": (C.c_int, [C.c_int, C.c_uint32, C.c_int, C.c_int, C.POINTER(Hyper), C.c_uint64, C.c_uint32, C.c_void_p,
                                 C.POINTER(C.c_void_p)]),
    "rp_nlhe_destroy": (C.c_int, [C.c_void_p]),
    "rp_nlhe_step": (C.c_int, [C.c_void_p, C.c_int]),
    "rp_nlhe_set_sampling": (C.c_int, [C.c_void_p, C.c_int]),
    "rp_nlhe_set_rng": (C.c_int, [C.c_void_p, C.c_int]),
    "rp_nlhe_set_exact": (C.c_int, [C.c_void_p, C.c_int]),
    "rp_kmeans_set_rng": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "rp_kmeans_set_libm": (C.c_int, [C.c_void_p, C.c_int]),
    "rp_kmeans_set_prune": (C.c_int, [C.c_void_p, C.c_int]),
    "rp_kmeans_prune_stats_sized": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "rp_nlhe_train": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_char_p, C.c_size_t]),
    "rp_nlhe_profile": (C.c_int, [C.c_void_p, C.c_int]),
    "rp_nlhe_kernel_time": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "rp_nlhe_census": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "rp_nlhe_last_shape": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rp_nlhe_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)] + [C.c_void_p] * 9),
    "rp_nlhe_epoch": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "rp_nlhe_counters": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "rp_nlhe_export": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rp_nlhe_import": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "rp_nlhe_capacity": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "rp_nlhe_resize": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rp_nlhe_set_growth": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64]),
    "rp_nlhe_export_device": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rp_nlhe_import_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "rp_nlhe_policy": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64] + [C.c_void_p] * 7),
    "rp_nlhe_policy_device": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64] + [C.c_void_p] * 7),
    "rp_nlhe_memory": (C.c_int, [C.c_void_p, C.c_uint64] + [C.c_void_p] * 6),
    "rp_nlhe_memory_device": (C.c_int, [C.c_void_p, C.c_uint64] + [C.c_void_p] * 6),
    "rp_nlhe_reaches": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint64] + [C.c_void_p] * 5),
    "rp_nlhe_reaches_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint64] + [C.c_void_p] * 5),
    "rp_nlhe_opponent_range": (C.c_int, [C.c_void_p, C.c_uint64] + [C.c_void_p] * 4),
    "rp_nlhe_opponent_range_device": (C.c_int, [C.c_void_p, C.c_uint64] + [C.c_void_p] * 4),
    "rp_nlhe_frontier_payoffs": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_float, C.c_uint32, C.c_uint64, C.c_uint64] + [C.c_void_p] * 3),
    "rp_nlhe_frontier_payoffs_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_float, C.c_uint32, C.c_uint64, C.c_uint64]
                                        + [C.c_void_p] * 3),
    "rp_nlhe_depth_args_default": (None, [C.POINTER(NlheDepthArgs)]),
    "rp_nlhe_depth_solve": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(NlheDepthArgs), C.c_void_p, C.c_void_p]),
    "rp_nlhe_depth_solve_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(NlheDepthArgs), C.c_void_p, C.c_void_p]),
    "rp_nlhe_subgame_args_default": (None, [C.POINTER(NlheSubgameArgs)]),
    "rp_nlhe_subgame_solve": (C.c_int, [C.c_void_p, C.c_uint64] + [C.c_void_p] * 4 + [C.POINTER(NlheSubgameArgs)] + [C.c_void_p] * 3),
    "rp_nlhe_subgame_solve_device": (C.c_int, [C.c_void_p, C.c_uint64] + [C.c_void_p] * 4 + [C.POINTER(NlheSubgameArgs)] + [C.c_void_p] * 3),
    "rp_nlhe_aivat": (C.c_int, [C.c_void_p, C.c_uint64] + [C.c_void_p] * 8),
    "rp_nlhe_aivat_device": (C.c_int, [C.c_void_p, C.c_uint64] + [C.c_void_p] * 8),
    "rp_aivat_summarize": (C.c_int, [C.c_uint64, C.c_void_p, C.c_float, C.POINTER(AivatSummary)]),
    "rp_nlhe_match_args_default": (None, [C.POINTER(NlheMatchArgs)]),
    "rp_nlhe_match": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(NlheMatchArgs)] + [C.c_void_p] * 4),
    "rp_nlhe_match_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(NlheMatchArgs)] + [C.c_void_p] * 4),
    "rp_nlhe_search_args_default": (None, [C.POINTER(NlheSearchArgs)]),
    "rp_nlhe_search_match": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(NlheSearchArgs)] + [C.c_void_p] * 7),
    "rp_nlhe_search_match_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(NlheSearchArgs)] + [C.c_void_p] * 7),
    "rp_match_summarize": (C.c_int, [C.c_uint64, C.c_void_p, C.POINTER(MatchSummary)]),
    "rp_nlhe_translate_args_default": (None, [C.POINTER(NlheTranslateArgs)]),
    "rp_nlhe_translate": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(NlheTranslateArgs)] + [C.c_void_p] * 10),
    "rp_nlhe_translate_device": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(NlheTranslateArgs)] + [C.c_void_p] * 10),
    "rp_nlhe_table_census": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rp_nlhe_table_census_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rp_census_stats": (C.c_int, [C.c_void_p, C.POINTER(CensusTotals)]),
    "rp_census_street_stats": (C.c_int, [C.c_void_p, C.POINTER(CensusStreet)]),
    "rp_census_saturation": (C.c_int, [C.c_void_p, C.POINTER(CensusPeaks)]),
    "rp_census_grid_usage": (C.c_int, [C.c_void_p, C.POINTER(CensusGrid), C.POINTER(C.c_uint32)]),
    "rp_nlhe_partition": (C.c_int, [C.c_void_p, C.c_uint64] + [C.c_void_p] * 4),
    "rp_nlhe_partition_device": (C.c_int, [C.c_void_p, C.c_uint64] + [C.c_void_p] * 4),
    "rp_nlhe_belief": (C.c_int, [C.c_void_p, C.c_uint64] + [C.c_void_p] * 5),
    "rp_nlhe_belief_device": (C.c_int, [C.c_void_p, C.c_uint64] + [C.c_void_p] * 5),
    "rp_nlhe_restrict": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64] + [C.c_void_p] * 4),
    "rp_nlhe_restrict_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64]
                                + [C.c_void_p] * 4),
    "rp_nlhe_set_shard": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "rp_nlhe_entry_bytes": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32)]),
    "rp_nlhe_step_local": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]),
    "rp_nlhe_step_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "rp_nlhe_step_comm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "rp_nlhe_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rp_nlhe_sync": (C.c_int, [C.c_void_p]),
    "rp_profile_set_rows": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "rp_nlhe_playouts": (C.c_int, [C.c_int, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rp_hand_strength": (C.c_int, [C.c_int, C.c_uint64, C.c_void_p, C.c_void_p]),
    "rp_obs_canonical": (C.c_int, [C.c_int, C.c_uint64, C.c_void_p, C.c_void_p]),
    "rp_isomorphisms": (C.c_int, [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "rp_river_equity": (C.c_int, [C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rp_lookup_create": (C.c_int, [C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "rp_lookup_destroy": (C.c_int, [C.c_void_p]),
    "rp_lookup_get": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "rp_lookup_project": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rp_deuce_kernel_ms": (C.c_int, [C.POINTER(C.c_double)]),
    "rp_atlas_create": (C.c_int, [C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "rp_atlas_destroy": (C.c_int, [C.c_void_p]),
    "rp_atlas_shape": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    "rp_atlas_tables": (C.c_int, [C.c_void_p] + [C.c_void_p] * 5),
    "rp_atlas_create_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    **{name + form: (C.c_int, [C.c_void_p, C.c_uint64] + args) for form in ("", "_device") for name, args in (
        ("rp_atlas_describe", [C.c_void_p] * 4),
        ("rp_atlas_obs_equity", [C.c_void_p] * 3),
        ("rp_atlas_pick", [C.c_void_p] * 4),
        ("rp_atlas_neighbors", [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
        ("rp_atlas_distance", [C.c_void_p] * 3),
        ("rp_atlas_histograms", [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
        ("rp_atlas_members", [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]))},
    "rp_pgcopy_write": (C.c_int, [C.c_char_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "rp_pgcopy_read": (C.c_int, [C.c_char_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "rp_artifact_write_lookup": (C.c_int, [C.c_char_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p]),
    "rp_artifact_write_abstraction": (C.c_int, [C.c_char_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]),
    "rp_artifact_write_isomorphism": (C.c_int, [C.c_char_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rp_artifact_write_metric": (C.c_int, [C.c_char_p, C.c_int, C.c_uint32, C.c_void_p]),
    "rp_artifact_write_blueprint": (C.c_int, [C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                              C.POINTER(C.c_uint64)]),
    "rp_artifact_write_transitions": (C.c_int, [C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
}

_lib = None


def load() -> C.CDLL:
    """Load librp_mi355x.so (once).  Raises if it has not been built: no silent fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C robopoker_amd/csrc).  The MI355X path has no CPU fallback."
        )
    # One HIP runtime per process: PyTorch ships its own libamdhip64, and whichever copy initialises the device first owns it —
    # a torch imported AFTER the library's first HIP call finds "No HIP GPUs".  Tests, bench.py and the multi-GPU harness all use
    # torch tensors for device buffers, so when torch is installed it is imported first, whatever order the callers import in.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(code: int) -> None:
    if code != RP_OK:
        raise RpError(code, load().rp_last_error().decode("utf-8", "replace"))


class Checkpoint(C.Structure):
    _fields_ = [("epoch", C.c_uint64), ("nodes", C.c_uint64), ("infos", C.c_uint64), ("rate", C.c_double)]


EVENT = C.CFUNCTYPE(None, C.c_int, C.c_void_p, C.c_char_p, C.c_void_p)


def train(fn, handle, *leading, max_steps=0, max_seconds=0.0, log_interval=60.0, flush_interval=1800.0, on_checkpoint=None,
          on_flush=None, interrupt=None) -> str:
    """rp_mccfr_train / rp_nlhe_train (``fn``) on ``handle``; ``leading`` are the arguments in front of max_steps.
    ``on_checkpoint(dict, line)`` gets the Checkpoint and its display line, ``on_flush(dict)`` fires at the flush cadence,
    ``interrupt`` is a ctypes c_int the caller may set to stop.  Returns Progress::summary."""

    def cb(event, cp, line, _user):
        c = C.cast(cp, C.POINTER(Checkpoint)).contents
        d = {"epoch": c.epoch, "nodes": c.nodes, "infos": c.infos, "rate": c.rate}
        if event == 0 and on_checkpoint:
            on_checkpoint(d, line.decode())
        if event == 1 and on_flush:
            on_flush(d)

    trampoline = EVENT(cb)
    buf = C.create_string_buffer(256)
    check(fn(handle, *leading, int(max_steps), float(max_seconds), float(log_interval), float(flush_interval),
             C.cast(trampoline, C.c_void_p), None, C.byref(interrupt) if interrupt is not None else None, buf, len(buf)))
    return buf.value.decode()


def kernel_time(fn, handle, name: str):
    """(total_ms, launches) of one of the handle's kernel clocks (``fn``: the handle's rp_*_kernel_time)"""
    ms, n = C.c_double(), C.c_uint64()
    check(fn(handle, name.encode(), C.byref(ms), C.byref(n)))
    return ms.value, n.value


def declared_symbols() -> list[str]:
    return sorted(_SIGNATURES)

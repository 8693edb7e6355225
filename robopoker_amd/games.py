"""Built-in game tables (crates/kuhn, crates/leduc, crates/roshambo) behind ``rp_game_*``."""
from __future__ import annotations

import ctypes as C

from . import _lib


class Game:
    """Owns an ``rp_game`` handle; ``table`` is the flat ``rp_game_table`` view passed to solvers."""

    def __init__(self, kind: str):
        lib = _lib.load()
        self.kind = kind
        self._h = C.c_void_p()
        _lib.check(lib.rp_game_create(_lib.GAME[kind], C.byref(self._h)))
        self.table = _lib.GameTable()
        _lib.check(lib.rp_game_view(self._h, C.byref(self.table)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            _lib.load().rp_game_destroy(h)
            self._h = None

    @property
    def n_infos(self) -> int:
        return self.table.n_infos

    @property
    def max_actions(self) -> int:
        return self.table.max_actions

    def hash_streams(self) -> _lib.HashStreams:
        """the `Hash::hash` byte stream of every infoset and in-tree chance info (reference-seed mode, Solver.set_rng)"""
        out = _lib.HashStreams()
        _lib.check(_lib.load().rp_game_hash_streams(self._h, C.byref(out)))
        return out

    def skeleton(self) -> str:
        """the compile-time action skeleton this table matches (csrc/traverse_static.hpp): "kuhn", "leduc" or "" — decides
        whether the solver's traversal is the instantiated kernel or the generic per-lane DFS; host-side check, no device"""
        out = C.c_int()
        _lib.check(_lib.load().rp_game_skeleton(C.byref(self.table), C.byref(out)))
        return ("", "kuhn", "leduc")[out.value]

    def info_id(self, name: str) -> int:
        out = C.c_uint32()
        _lib.check(_lib.load().rp_game_info_id(self._h, name.encode(), C.byref(out)))
        return out.value

    def info_name(self, info: int) -> str:
        buf = C.create_string_buffer(64)
        _lib.check(_lib.load().rp_game_info_name(self._h, info, buf, 64))
        return buf.value.decode()

    def n_actions(self, info: int) -> int:
        return self.table.info_actions[info]

    def player(self, info: int) -> int:
        return self.table.info_player[info]


# ---- entries of the safe subgame re-solve (Solver.subgame_belief / subgame_solve) for the built-in Kuhn and Leduc ---------------------
_CARDS = {"kuhn": 6, "leduc": 6, "leduc_wide": 14}  # Card::ALL = two suits per rank, rank = card // 2


def _child(table, state: int, slot: int) -> int:
    st = table.states[state]
    if slot >= st.n_children:
        raise ValueError(f"state {state} has no child slot {slot}")
    return table.children[st.offset + slot]


def deal_state(game: Game, holes) -> int:
    """the first decision state after the two private cards `holes` = (seat 0's, seat 1's), Card::ALL indices"""
    c0, c1 = holes
    if c0 == c1:
        raise ValueError("the two hole cards must differ")
    t = game.table
    return _child(t, _child(t, t.train_root, c0), c1 - (1 if c1 > c0 else 0))


def play(game: Game, holes, prefix) -> int:
    """the state after `prefix` from deal_state(holes): an int is an action slot, ("board", card) the Leduc board deal"""
    s = deal_state(game, holes)
    for step in prefix:
        if isinstance(step, tuple):
            card = step[1]
            if card in holes:
                raise ValueError("the board card is one of the hole cards")
            step = card - sum(1 for h in holes if h < card)
        s = _child(game.table, s, step)
    return s


def harvest_order(game: Game, info: int):
    """the slots of `info` in the derived Ord of the game's edge enum: Kuhn Check < Bet < Call < Fold (kuhn/src/edge.rs:10-16) against
    the slot order [Fold, Call] of a bet-facing infoset; Leduc Fold < Check < Call < Raise agrees with both of its slot orders"""
    order = list(range(16))
    if game.kind == "kuhn" and game.info_name(info).split("|")[1] in ("B", "XB"):
        order[0], order[1] = 1, 0
    return order


def subgame_entry(game: Game, holes, prefix=(), external=1, reach=False, n_worlds=2, harvest_info=None):
    """-> (prior, entry) records (mccfr.SUBGAME_PRIOR_DTYPE / SUBGAME_ENTRY_DTYPE, one element each) for the subgame at the state after
    `prefix`, as the reference's tests build them (kuhn/src/solver.rs:318-517, leduc/src/solver.rs:165-285).  The candidates are
    Card::ALL minus the other seat's card and the board, in that order, `external` holding each in turn (the encoders' `restrict`), the
    secret a card's rank.  reach = False is `baseline` (mass 1 per candidate); reach = True conditions on the prefix: each candidate's
    root is its deal and the path the prefix (Solver::external_reach) — a prefix with a board deal has no shared path and is refused.
    entry.world_of / weights are left for Solver.subgame_belief's answer (see fill_belief)."""
    import numpy as np

    from .mccfr import SUBGAME_ENTRY_DTYPE, SUBGAME_PRIOR_DTYPE

    if game.kind not in _CARDS:
        raise ValueError("subgame_entry knows the built-in card games only")
    holes, internal = tuple(holes), 1 - external
    board = [step[1] for step in prefix if isinstance(step, tuple)]
    cards = [c for c in range(_CARDS[game.kind]) if c != holes[internal] and c not in board]
    if len(cards) > 16:
        raise ValueError("more than 16 candidates")
    with_card = [tuple(c if seat == external else holes[seat] for seat in (0, 1)) for c in cards]
    prior, entry = np.zeros(1, SUBGAME_PRIOR_DTYPE), np.zeros(1, SUBGAME_ENTRY_DTYPE)
    p, e = prior[0], entry[0]
    p["n_prior"], p["internal"], p["mode"], p["n_worlds"] = len(cards), internal, 1 if reach else 0, n_worlds
    p["secret"][:len(cards)] = [c // 2 for c in cards]
    if reach:
        if board:
            raise ValueError("a reach-conditioned prior needs a prefix without a board deal")
        p["root_state"][:len(cards)] = [deal_state(game, h) for h in with_card]
        p["path"][:len(prefix)], p["n_path"] = list(prefix), len(prefix)
    else:
        p["root_state"][:len(cards)] = [play(game, h, prefix) for h in with_card]
    e["observed"], e["external"], e["n_candidates"], e["n_worlds"] = play(game, holes, prefix), external, len(cards), n_worlds
    e["candidate"][:len(cards)] = [play(game, h, prefix) for h in with_card]
    e["secret"][:len(cards)] = [c // 2 for c in cards]
    e["world_of"][:] = _lib.RP_WORLD_NONE
    e["harvest_info"] = _lib.RP_NO_INFO if harvest_info is None else harvest_info
    st = game.table.states[int(e["observed"])]
    shown = harvest_info if harvest_info is not None else (st.info if st.turn < 2 else None)
    e["harvest_order"][:] = harvest_order(game, shown) if shown is not None else list(range(16))
    return prior, entry


def frontiers(game: Game) -> dict:
    """rp_game_frontiers: the reference's frontier tables of a built-in game, as Solver.set_frontiers takes them —
    {"depth" u8 [n_states], "pick_info" u32 [n_states], "payoff_ref" u32 [n_states], "n_pick"}"""
    import numpy as np

    n = game.table.n_states
    out = {"depth": np.zeros(n, np.uint8), "pick_info": np.zeros(n, np.uint32), "payoff_ref": np.zeros(n, np.uint32)}
    n_pick = C.c_uint32()
    _lib.check(_lib.load().rp_game_frontiers(game._h, out["depth"].ctypes.data, out["pick_info"].ctypes.data, out["payoff_ref"].ctypes.data,
                                             C.byref(n_pick)))
    out["n_pick"] = n_pick.value
    return out


def depth_entry(game: Game, holes, prefix=(), internal=0):
    """-> entry record (mccfr.SUBGAME_ENTRY_DTYPE, one element) of ``DepthSolver::new(source, prefix, internal, entry)`` at the state
    after `prefix`: no candidates, one world of weight 1, external = 1 - internal.  Solver.depth_solve(entry) (origin None: the
    entry state's depth) is that solver's steps and harvest."""
    import numpy as np

    from .mccfr import SUBGAME_ENTRY_DTYPE

    if game.kind not in _CARDS:
        raise ValueError("depth_entry knows the built-in card games only")
    entry = np.zeros(1, SUBGAME_ENTRY_DTYPE)
    e = entry[0]
    e["observed"], e["external"], e["n_candidates"], e["n_worlds"] = play(game, tuple(holes), prefix), 1 - internal, 0, 1
    e["weights"] = (1, 0, 0, 0)
    e["world_of"][:] = _lib.RP_WORLD_NONE
    e["harvest_info"] = _lib.RP_NO_INFO
    st = game.table.states[int(e["observed"])]
    e["harvest_order"][:] = harvest_order(game, st.info) if st.turn < 2 else list(range(16))
    return entry


def fill_belief(entries, belief):
    """copies Solver.subgame_belief's answer (or the model's) into the entries, element by element"""
    entries["world_of"][...] = belief["world_of"]
    entries["weights"][...] = belief["weights"]
    return entries

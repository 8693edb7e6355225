"""Caller-built rp_game_table's for the dense MCCFR solver.  TEST INFRASTRUCTURE ONLY.

rp_mccfr_create takes any rp_game_table; the built-in games (Kuhn, Leduc, RPS, wide Leduc) are all two-player, zero-sum, at most
three actions wide and small enough for the LDS traversal.  TableGame builds the tables a downstream trainer could hand over
instead, from a list of layers, and CATALOGUE names the ones the tests traverse: each exists for one path of the kernels and states
which traversal kernel (rp_mccfr_traversal_variant) it must select.

A plan is a list of layers, applied in order to every history that has not ended:
    ("deal", player, n)                 a private chance node: only `player` sees which of the n outcomes was dealt
    ("chance", n)  /  ("chance", n, True)  a public chance node; True: it carries a chance_info (reference-seed mode draws it from
                                        its own hash stream, rp_hash_streams.chance)
    ("act", player, n)  /  ("act", player, n, stop)
                                        a decision of `player` over n public actions; action `stop` (if given) ends the game
`player` and `n` may be callables of the public history (a tuple of (layer, outcome) pairs); n == 0 skips the layer for that
history.  After the last layer the game ends.

Infosets are (player, layer, public history, own private deals), numbered on first visit: perfect recall and one action count per
infoset by construction.  Terminal payoffs are multiples of 0.25 in [-2, 2] from a CRC of the whole path, one per player and not
zero-sum.  States are emitted in pre-order, so children follow parents (rp_game_table_check).
"""
from __future__ import annotations

import ctypes as C
import struct
import sys
import zlib

import numpy as np

from robopoker_amd import _lib

CHANCE, TERMINAL, NO_INFO = _lib.RP_TURN_CHANCE, _lib.RP_TURN_TERMINAL, _lib.RP_NO_INFO


class TableGame:
    """an rp_game_table in ctypes, with what Solver / OracleSolver read from a robopoker_amd.Game"""

    def __init__(self, n_players, plan, default_regret=None, seed=0):
        self.n_players, self.plan, self.seed = n_players, plan, seed
        self.turn, self.nch, self.info, self.offset, self.chance_info = [], [], [], [], []
        self.children, self.payoffs = [], []
        self.info_actions, self.info_player, self._info_ids, self._chance_ids = [], [], {}, {}
        limit = sys.getrecursionlimit()
        sys.setrecursionlimit(max(limit, 10000))
        try:
            self._emit(0, (), tuple(() for _ in range(n_players)), ())
        finally:
            sys.setrecursionlimit(limit)
        self._freeze(default_regret)

    # ---- construction -----------------------------------------------------------------------------------------------------------
    def _emit(self, layer, pub, priv, path):
        """the state reached by `path`; returns its index.  Pre-order: the state is appended before its children."""
        while layer < len(self.plan):
            kind = self.plan[layer][0]
            n = self.plan[layer][2 if kind != "chance" else 1]
            n = n(pub) if callable(n) else n
            if n:
                break
            layer += 1  # a layer this history skips
        me = len(self.turn)
        if layer == len(self.plan):
            return self._terminal(path)
        spec = self.plan[layer]
        for arr, v in ((self.turn, CHANCE), (self.nch, n), (self.info, NO_INFO), (self.offset, len(self.children)), (self.chance_info, 0)):
            arr.append(v)
        first = len(self.children)
        self.children.extend([0xFFFFFFFF] * n)
        if kind == "deal":
            who = spec[1]
            for k in range(n):
                dealt = tuple(h + ((layer, k),) if p == who else h for p, h in enumerate(priv))
                self.children[first + k] = self._emit(layer + 1, pub, dealt, path + (k,))
        elif kind == "chance":
            if len(spec) > 2 and spec[2]:
                self.chance_info[me] = self._chance_ids.setdefault((layer, pub), len(self._chance_ids) + 1)
            for k in range(n):
                self.children[first + k] = self._emit(layer + 1, pub + ((layer, k),), priv, path + (k,))
        else:
            who = spec[1](pub) if callable(spec[1]) else spec[1]
            stop = spec[3] if len(spec) > 3 else None
            key = (who, layer, pub, priv[who])
            if key not in self._info_ids:
                self._info_ids[key] = len(self.info_actions)
                self.info_actions.append(n)
                self.info_player.append(who)
            self.turn[me], self.info[me] = who, self._info_ids[key]
            for k in range(n):
                if k == stop:
                    self.children[first + k] = self._terminal(path + (k,))
                else:
                    self.children[first + k] = self._emit(layer + 1, pub + ((layer, k),), priv, path + (k,))
        return me

    def _terminal(self, path):
        me = len(self.turn)
        for arr, v in ((self.turn, TERMINAL), (self.nch, 0), (self.info, NO_INFO), (self.offset, len(self.payoffs) // self.n_players),
                       (self.chance_info, 0)):
            arr.append(v)
        for p in range(self.n_players):
            crc = zlib.crc32(bytes(path) + bytes([255, p]), self.seed)
            self.payoffs.append(0.25 * (crc % 17 - 8))
        return me

    def _freeze(self, default_regret):
        n = len(self.turn)
        self._states = (_lib.State * n)()
        for i in range(n):
            s = self._states[i]
            s.turn, s.n_children, s.chance_info, s.info, s.offset = self.turn[i], self.nch[i], self.chance_info[i], self.info[i], self.offset[i]
        self._children = (C.c_uint32 * max(len(self.children), 1))(*self.children)
        self._payoffs = (C.c_float * len(self.payoffs))(*self.payoffs)
        self._info_actions = (C.c_uint8 * len(self.info_actions))(*self.info_actions)
        self._info_player = (C.c_uint8 * len(self.info_player))(*self.info_player)
        A = max(self.info_actions)
        self._default_regret = None
        if default_regret is not None:
            # CfrEdge::default_regret: what a missing table entry reads.  Multiples of 1/8 in [-1, 1] from a CRC of the cell
            dr = np.zeros((len(self.info_actions), A), dtype=np.float32)
            for i, na in enumerate(self.info_actions):
                for a in range(na):
                    dr[i, a] = 0.125 * (zlib.crc32(struct.pack("<II", i, a), default_regret) % 17 - 8)
            self.default_regret = dr
            self._default_regret = (C.c_float * dr.size)(*dr.ravel())
        b = self.bounds()
        self.max_depth, self.max_tree_nodes = b["depth"], b["nodes"]
        self.table = self.make_table()

    def make_table(self, **overrides):
        """a GameTable over this object's arrays (which stay alive with it); overrides replace scalar fields"""
        t = _lib.GameTable()
        t.n_states, t.n_infos, t.n_players = len(self.turn), len(self.info_actions), self.n_players
        t.max_actions = max(self.info_actions)
        t.n_children, t.n_terminals = len(self.children), len(self.payoffs) // self.n_players
        t.train_root = t.exploit_root = 0
        t.max_depth, t.max_tree_nodes = self.max_depth, self.max_tree_nodes
        t.states = self._states
        t.children = self._children
        t.payoffs = self._payoffs
        t.info_actions = self._info_actions
        t.info_player = self._info_player
        if self._default_regret is not None:
            t.default_regret = self._default_regret
        for k, v in overrides.items():
            setattr(t, k, v)
        return t

    # ---- bounds, independently of csrc/games.cpp ----------------------------------------------------------------------------------
    def bounds(self):
        """longest root-to-leaf path (states) and, as the maximum over the walkers, of one externally sampled tree (walker states keep
        every child, all other states one): its nodes, its internal (expanded) nodes and the pending leaves of a pop-last DFS that
        pushes every kept child and pops one (+ 1: the library's own margin).  Explicit post-order over the states, no recursion."""
        n = len(self.turn)
        kids = [self.children[self.offset[s]:self.offset[s] + self.nch[s]] for s in range(n)]
        depth = [1] * n
        for s in reversed(range(n)):  # pre-order emission: every child has a larger index than its parent
            if kids[s]:
                depth[s] = 1 + max(depth[c] for c in kids[s])
        out = dict(depth=depth[0], nodes=0, internal=0, stack=0)
        for w in range(self.n_players):
            nodes, internal, stack = [1] * n, [0] * n, [0] * n
            for s in reversed(range(n)):
                if not kids[s]:
                    continue
                fold = sum if self.turn[s] == w else max
                nodes[s] = 1 + fold(nodes[c] for c in kids[s])
                internal[s] = 1 + fold(internal[c] for c in kids[s])
                kept = len(kids[s]) if self.turn[s] == w else 1
                stack[s] = kept - 1 + max(1, max(stack[c] for c in kids[s]))
            out["nodes"] = max(out["nodes"], nodes[0])
            out["internal"] = max(out["internal"], internal[0])
            out["stack"] = max(out["stack"], stack[0])
        out["internal"] = max(out["internal"], 1)
        out["stack"] = max(out["stack"], 1) + 1
        return out

    def expected_variant(self):
        """rp_mccfr_traversal_variant as the documented limits of the LDS traversal predict it (include/rp_mi355x.h,
        csrc/mccfr_traverse.hpp): 1 when a sampled tree has at most 62 nodes and 32 internal nodes, the game at most depth 10, 8191
        infosets and 16 actions, and two dwords per node + the stack (or two reach prefixes per internal node) + one value per action
        (more than 4 actions) fit 64 KB for 64 lanes; 0 (scratch in HBM) otherwise.  None of these tables matches a skeleton."""
        b, A = self.bounds(), self.max_actions
        words = 2 * b["nodes"] + max(2 * b["internal"], 4 * b["stack"]) + (0 if A <= 4 else A)
        fits = b["nodes"] <= 62 and b["internal"] <= 32 and b["depth"] <= 10 and self.n_infos <= 8191 and A <= 16 and words * 256 <= 65536
        return 1 if fits else 0

    # ---- what Solver / OracleSolver read from a Game ------------------------------------------------------------------------------
    @property
    def n_infos(self):
        return len(self.info_actions)

    @property
    def max_actions(self):
        return max(self.info_actions)

    def n_actions(self, info):
        return self.info_actions[info]

    def player(self, info):
        return self.info_player[info]

    def info_of(self, key):
        """the id of infoset (player, layer, public history, own private deals)"""
        return self._info_ids[key]

    def hash_streams(self):
        """caller-built rp_hash_streams: an infoset writes its id as 4 little-endian bytes, an in-tree chance info b"c" and its
        index — any injective choice serves, the device and the oracle are handed the same bytes"""
        def stream(data):
            s = _lib.HashStream()
            s.len = len(data)
            for i, byte in enumerate(data):
                s.bytes[i] = byte
            return s

        self._info_streams = (_lib.HashStream * self.n_infos)(*[stream(struct.pack("<I", i)) for i in range(self.n_infos)])
        n_chance = len(self._chance_ids)
        self._chance_streams = (_lib.HashStream * max(n_chance, 1))(*[stream(b"c" + struct.pack("<I", i)) for i in range(max(n_chance, 1))])
        out = _lib.HashStreams()
        out.n_infos, out.n_chance = self.n_infos, n_chance
        out.infos, out.chance = self._info_streams, self._chance_streams
        return out


# ---- the catalogue ------------------------------------------------------------------------------------------------------------
def _first_action(layer):
    return lambda pub: next(k for l, k in pub if l == layer)


# name -> (why the game exists, players, plan, default_regret seed or None, the traversal variant it must select)
_SPECS = {
    # k_traverse_lds<false> (5..16 actions: values in LDS), payoffs[off * 3 + walker], walker = epoch % 3, three owners in
    # rank_count / rank_info; 1-, 2-, 3- and 5-action infosets in one game; a terminating action
    "three_players_a5": ("three players, 1/2/3/5 actions, mid-tree public chance", 3,
                         [("deal", 0, 2), ("deal", 1, 2), ("deal", 2, 2), ("act", 0, 3, 0), ("act", 1, 2), ("chance", 3),
                          ("act", 2, lambda pub: 5 if pub[-1][1] == 0 else 2), ("act", 0, 1)], None, 1),
    # the widest row everywhere (traversal, k_prepare_infos, chains, block maps); > 256 infosets: the large-game update kernels
    "widest_a16": ("a 16-action infoset, default_regret set, 336 infosets", 2,
                   [("chance", 4), ("deal", 0, 4), ("deal", 1, 5), ("act", 0, 16), ("act", 1, 2)], 7, 1),
    "one_player": ("one player: chance, player, chance, player", 1,
                   [("chance", 4), ("act", 0, 3), ("chance", 3), ("act", 0, 2)], None, 1),
    "chance16_mid": ("a 16-way chance node below a walker node and above an opponent node", 2,
                     [("deal", 0, 3), ("deal", 1, 3), ("act", 0, 2), ("chance", 16, True), ("act", 1, 3), ("act", 0, 2)], None, 1),
    "two_states": ("one 1-action player node over one terminal: player root, no chance", 2, [("act", 0, 1)], None, 1),
    # max_depth 10 / 11: private deals, then action 0 folds and action 1 goes on
    "depth10": ("depth 10, the deepest game of the LDS traversal", 2,
                [("deal", 0, 3), ("deal", 1, 3)] + [("act", k % 2, 2, 0) for k in range(7)], None, 1),
    "depth11": ("depth 11: one layer past the LDS traversal", 2,
                [("deal", 0, 3), ("deal", 1, 3)] + [("act", k % 2, 2, 0) for k in range(8)], None, 0),
    # walker 0's tree: chance, opponent, root + 4 + (14 + 14 + 14 + 13 | 14) leaves
    "nodes62": ("a 62-node sampled tree, the largest of the LDS traversal", 2,
                [("chance", 3), ("act", 1, 2), ("act", 0, 4), ("act", 0, lambda pub: 13 if pub[-1][1] == 3 else 14)], None, 1),
    "nodes63": ("a 63-node sampled tree: one node past the LDS traversal", 2,
                [("chance", 3), ("act", 1, 2), ("act", 0, 4), ("act", 0, 14)], None, 0),
    # walker 0's tree: chance, root, 5 chains of 6 one-action nodes (+ one more node on the first chain)
    "internal32": ("32 internal nodes in a sampled tree, the most of the LDS traversal", 2,
                   [("chance", 3), ("act", 0, 5)] + [("act", (k + 1) % 2, 1) for k in range(6)], None, 1),
    "internal33": ("33 internal nodes: one past the LDS traversal", 2,
                   [("chance", 3), ("act", 0, 5)] + [("act", (k + 1) % 2, 1) for k in range(6)]
                   + [("act", 1, lambda pub: 1 if _first_action(1)(pub) == 0 else 0)], None, 0),
    # chance levels of at most 16 outcomes (the fan-out limit) over one 2-action node per path; the acting player alternates with
    # the last outcome, so both walkers decide
    "infos8191": ("8191 infosets, the most the LDS traversal's node word can name", 2,
                  [("chance", 16), ("chance", 16), ("chance", 16), ("chance", lambda pub: 1 if pub == ((0, 15), (1, 15), (2, 15)) else 2),
                   ("act", lambda pub: pub[-1][1] ^ (pub[-2][1] & 1), 2)], None, 1),
    "infos8192": ("8192 infosets: one past the LDS traversal", 2,
                  [("chance", 16), ("chance", 16), ("chance", 16), ("chance", 2), ("act", lambda pub: pub[-1][1] ^ (pub[-2][1] & 1), 2)],
                  None, 0),
    # not part of the parity sweep: the exact chance-draw counts
    "chance16_root": ("a 16-way root chance over one walker infoset per outcome", 2, [("chance", 16), ("act", 0, 2)], None, 1),
}

CATALOGUE = {name: dict(why=why, players=players, variant=variant) for name, (why, players, plan, dr, variant) in _SPECS.items()}
_built = {}


def game(name) -> TableGame:
    """the catalogue's game, built once per process (tests never modify one)"""
    if name not in _built:
        why, players, plan, dr, variant = _SPECS[name]
        _built[name] = TableGame(players, plan, default_regret=dr, seed=zlib.crc32(name.encode()))
    return _built[name]

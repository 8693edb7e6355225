"""CfrNash::exploitability (crates/mccfr/src/strategy/nash.rs:31-38,103-194) restated in numpy.  TEST INFRASTRUCTURE, not a test.

It reads a game through the ctypes rp_game_table that robopoker_amd.Game and game_tables.game expose, and a table as Solver.export /
OracleSolver.export return it, and gives the best response with its parts: exploitability, values [n_players], choice [n_infos],
cfv [n_infos, max_actions] — what rp_mccfr_best_response returns.  tests/test_nash_model.py pins its scalar to the oracle's.

Every sum and product is a sequential f32 fold in the reference's order: numpy's elementwise float32 + * / are IEEE single
operations, and the folds below advance one operand at a time (over k, over the walk to the root, over a span) while numpy only runs
the independent nodes, or cells, side by side.  np.sum / np.prod (pairwise) are not used.
"""
from __future__ import annotations

import numpy as np

CHANCE = 254
EPS = np.float32(1.17549435e-38)  # pokerkit::EPSILON = f32::MIN_POSITIVE
F0, F1 = np.float32(0.0), np.float32(1.0)


class Tree:
    """the VanillaSampling expansion from exploit_root in TreeBuilder's pop-last order (builder.rs:141-161)"""

    def __init__(self, table):
        t = table
        self.n_players, self.n_infos, self.A = t.n_players, t.n_infos, t.max_actions
        st_turn = np.array([t.states[i].turn for i in range(t.n_states)], dtype=np.int64)
        st_nch = np.array([t.states[i].n_children for i in range(t.n_states)], dtype=np.int64)
        st_info = np.array([t.states[i].info for i in range(t.n_states)], dtype=np.int64)
        st_off = np.array([t.states[i].offset for i in range(t.n_states)], dtype=np.int64)
        children = np.array(t.children[: t.n_children], dtype=np.int64)
        self.payoffs = np.array(t.payoffs[: t.n_terminals * t.n_players], dtype=np.float32)
        self.info_actions = np.array(t.info_actions[: t.n_infos], dtype=np.int64)
        self.info_player = np.array(t.info_player[: t.n_infos], dtype=np.int64)
        state, parent, edge, depth = [], [], [], []
        todo = [(t.exploit_root, -1, -1)]
        while todo:
            s, p, e = todo.pop()
            me = len(state)
            state.append(s)
            parent.append(p)
            edge.append(e)
            depth.append(depth[p] + 1 if p >= 0 else 0)
            todo.extend((int(children[st_off[s] + k]), me, k) for k in range(st_nch[s]))
        self.n = len(state)
        state = np.array(state, dtype=np.int64)
        self.parent, self.edge, self.depth = (np.array(x, dtype=np.int64) for x in (parent, edge, depth))
        self.turn, self.nch, self.info, self.off = st_turn[state], st_nch[state], st_info[state], st_off[state]
        self.kids = np.full((self.n, max(int(self.nch.max()), 1)), -1, dtype=np.int64)
        has = self.parent >= 0
        self.kids[self.parent[has], self.edge[has]] = np.nonzero(has)[0]
        self.levels = [np.nonzero(self.depth == d)[0] for d in range(int(self.depth.max()) + 1)]


def averaged(tree: Tree, weight: np.ndarray) -> np.ndarray:
    """avg[info][a] = max(w, EPS) / sum_k max(w_k, EPS), the sum from +0.0 over ascending k (profile.rs:40-44)"""
    wt = np.maximum(weight.reshape(tree.n_infos, tree.A).astype(np.float32), EPS)
    total = np.zeros(tree.n_infos, dtype=np.float32)
    for k in range(tree.A):
        total = np.where(k < tree.info_actions, total + wt[:, k], total)
    return wt / total[:, None]


def values(tree: Tree, avg: np.ndarray, hero: int, choice=None) -> np.ndarray:
    """v[node] bottom-up by level; with `choice`, hero nodes take the chosen kid's value"""
    v = np.zeros(tree.n, dtype=np.float32)
    for nodes in reversed(tree.levels):
        nch, turn = tree.nch[nodes], tree.turn[nodes]
        leaf = nodes[nch == 0]
        v[leaf] = tree.payoffs[tree.off[leaf] * tree.n_players + hero]
        inner = nodes[nch > 0]
        if inner.size == 0:
            continue
        nch, turn, info = tree.nch[inner], tree.turn[inner], tree.info[inner]
        chance = turn == CHANCE
        s = np.zeros(inner.size, dtype=np.float32)
        for k in range(int(nch.max())):
            live = k < nch
            kid = np.where(live, tree.kids[inner, k], 0)
            w = np.where(chance, F1, avg[np.where(chance, 0, info), min(k, tree.A - 1)])
            # a chance node adds the kid's value itself, a player node avg * v
            s = np.where(live, s + np.where(chance, v[kid], w * v[kid]), s)
        s = np.where(chance, s / nch.astype(np.float32), s)
        if choice is not None:
            mine = turn == hero
            picked = tree.kids[inner, np.where(mine, choice[np.where(chance, 0, info)], 0)]
            s = np.where(mine, v[picked], s)
        v[inner] = s
    return v


def best_response(table, rows) -> dict:
    tree = Tree(table)
    avg = averaged(tree, rows["weight"])
    cfv = np.zeros((tree.n_infos, tree.A), dtype=np.float32)
    choice = np.zeros(tree.n_infos, dtype=np.int64)
    vals = np.zeros(tree.n_players, dtype=np.float32)
    ties = 0
    for hero in range(tree.n_players):
        v = values(tree, avg, hero)
        # external_reach of every child of a hero node: from 1.0, multiplied leaf to root by avg[parent.info][edge] at every parent
        # that is neither chance nor the hero's
        kid = np.nonzero((tree.parent >= 0) & (tree.turn[np.maximum(tree.parent, 0)] == hero))[0]
        p = np.ones(kid.size, dtype=np.float32)
        cur = kid.copy()
        while True:
            par = tree.parent[cur]
            up = par >= 0
            if not up.any():
                break
            par0 = np.where(up, par, 0)
            opp = up & (tree.turn[par0] != CHANCE) & (tree.turn[par0] != hero)
            f = avg[np.where(opp, tree.info[par0], 0), np.where(opp, tree.edge[cur], 0)]
            p = np.where(opp, p * f, p)
            cur = np.where(up, par, cur)
        term = np.zeros(tree.n, dtype=np.float32)
        term[kid] = p * v[kid]
        # cfv[info][a] over the span in ascending node index: the j-th node of every span side by side
        mine = np.nonzero((tree.turn == hero) & (tree.nch > 0))[0]
        order = mine[np.argsort(tree.info[mine], kind="stable")]
        infos = tree.info[order]
        first = np.r_[0, np.nonzero(np.diff(infos))[0] + 1] if order.size else np.zeros(0, dtype=np.int64)
        pos = np.arange(order.size) - np.repeat(first, np.diff(np.r_[first, order.size]))
        for j in range(int(pos.max()) + 1 if order.size else 0):
            sel = order[pos == j]
            for a in range(tree.A):
                m = sel[a < tree.nch[sel]]
                cfv[tree.info[m], a] = cfv[tree.info[m], a] + term[tree.kids[m, a]]
        owned = np.nonzero(tree.info_player == hero)[0]
        best = cfv[owned, 0].copy()
        pick = np.zeros(owned.size, dtype=np.int64)
        for a in range(1, tree.A):
            with np.errstate(invalid="ignore"):
                ge = (a < tree.info_actions[owned]) & (cfv[owned, a] >= best)  # max_by keeps the last maximum (nash.rs:184-193)
            ties += int((ge & (cfv[owned, a] == best)).sum())
            best = np.where(ge, cfv[owned, a], best)
            pick = np.where(ge, a, pick)
        choice[owned] = pick
        vals[hero] = values(tree, avg, hero, choice)[0]
    total = F0
    for hero in range(tree.n_players):
        total = total + vals[hero]
    return {"exploitability": np.float32(total / np.float32(tree.n_players)), "values": vals, "choice": choice.astype(np.uint8), "cfv": cfv,
            "ties": ties, "nodes": tree.n}

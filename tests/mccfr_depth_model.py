"""The model the table-game depth-limited tests compare against (helper, no tests): rp_mccfr_depth_solve (include/rp_mi355x.h) by the
NAIVE algorithm of the reference's text, twice over —

  WithOrigin   SubGameSolver::with_origin (subgame/src/solver.rs: build(.., Some(origin)), step, Harvest::harvest) over WorldProfile
               over DepthView: mccfr_subgame_model.Solve's worlds, restrict and harvest with the frontier machinery below switched on;
  DepthSolver  DepthSolver::new / step / harvest (subgame/src/depth/solver.rs:21-123) on their own: no world, no belief, a fixed
               entry state, origin = Some(entry.depth()), the profile keyed by DepthInfo alone.

Both grow their trees through `Flow`: DepthGame::at_frontier / apply / payoff (depth/game.rs), DepthEncoder::branches and its Pick
infosets (depth/encoder.rs:93-121), DepthView's constants for Pick edges (depth/view.rs), TreeBuilder with ExternalSampling (a chance
node keeps one branch uniformly), CfrFlow::dfs / recursed_value / ancestor_reach (a chance node multiplies no reach) and
CfrNash::terminal_value.  Recursion, dicts, np.float32 scalars with one rounding per operation.  The kernel
(robopoker_amd/csrc/mccfr_subgame.hpp, FR = true) keeps a kind per node, numbers a Pick infoset n_infos + pick id and sweeps the
tree level by level, so that this checks it."""
from __future__ import annotations

import numpy as np

import mccfr_subgame_model as M
from mccfr_subgame_model import CHANCE, ENC, EPS, MAX_ITERATIONS, MAX_NODES, MAX_ROWS, NO_INFO, OK, ROWS, TERMINAL, TREE, F, M64, Malformed, fold, node_hash, u01

FRONTIER = 13  # RP_MSUB_FRONTIER
ORIGIN_ENTRY, ORIGIN_NONE = 254, 255
GAME, PICK = 0, 1  # the kind of an infoset
N_GAME, N_FRONTIER, N_INTERNAL, N_EXTERNAL = range(4)  # the kind of a node


def pick_uniform(h, n):
    return (((h >> 32) * n) & M64) >> 32


class Frontiers:
    """the handle's frontier tables: depth, pick_info, payoff_ref per state, the matrices, D"""

    def __init__(self, depth, pick_info, payoff_ref, matrices=None, leaves=4, n_pick=None):
        self.depth, self.pick_info, self.payoff_ref = [int(x) for x in depth], [int(x) for x in pick_info], [int(x) for x in payoff_ref]
        self.matrices = np.zeros((0, leaves, leaves), F) if matrices is None else np.asarray(matrices, F)
        self.D = leaves
        named = [p for p in self.pick_info if p != NO_INFO]
        self.n_pick = n_pick if n_pick is not None else (max(named) + 1 if named else 0)

    def payoffs(self, table, bp, state):
        """DepthSampler::payoffs at a frontier state: [k][j] to `internal`; None where the tables name nothing"""
        ref, D = self.payoff_ref[state], self.D
        if ref == NO_INFO:
            return [[F(0.0)] * D for _ in range(D)]  # Payoffs::uniform(0.0)
        if ref & 0x80000000:
            m = ref & 0x7FFFFFFF
            return [[F(self.matrices[m, k, j]) for j in range(D)] for k in range(D)] if m < len(self.matrices) else None
        if ref < table.n_infos:  # Payoffs::uniform(blueprint.frontier_payoff(info)): cum_payoff(info, first choice) of the BLUEPRINT
            return [[F(bp.get(ref, 0, "payoff"))] * D for _ in range(D)]
        return None


class Profile(M.Profile):
    """DepthProfile over DepthView (WorldProfile over them when the key carries a world): key = (.., kind, id)"""

    def __init__(self, table, bp, hyper, prior, D):
        super().__init__(table, bp, hyper, prior)
        self.D = D

    def n(self, key):
        return self.D if key[-2] == PICK else self.table.actions[key[-1]]

    def cum(self, key, a, field):
        e = self.local.get(key, {}).get(a)
        if e is not None:
            return e[field]
        if key[-2] == PICK:  # DepthView: weight 1 / D, regret EPSILON, payoff 0, visits 0
            return {"weight": F(F(1.0) / F(self.D)), "regret": EPS, "payoff": F(0.0), "visits": 0}[field]
        v = self.bp.get(key[-1], a, field)
        return np.fmax(v, EPS) if field in ("weight", "regret") else v

    def mut(self, key, a):
        edges = self.local.setdefault(key, {})
        if a not in edges:
            if key[-2] == PICK:  # DepthView::warmstart of a Pick edge: Encounter::default()
                edges[a] = {"weight": F(0.0), "regret": F(0.0), "payoff": F(0.0), "visits": 0}
            else:
                k = self.prior
                with np.errstate(all="ignore"):
                    p = self.bp.averaged(key[-1], self.n(key))[a]
                    edges[a] = {"weight": F(F(F(p * k) * F(k + F(1.0))) / F(2.0)), "regret": F(0.0), "payoff": F(0.0), "visits": 0}
        return edges[a]


class Node(M.Node):
    def __init__(self, index, state, parent, slot, kind, turn, key):
        super().__init__(index, state, parent, slot)
        self.kind, self.turn, self.key = kind, turn, key


class Flow:
    """the tree, the values and the updates of one iteration; `self.tag` is the prefix of every infoset key (the world, or nothing)"""

    def grow(self, entry_state, walker):
        T, p, fr = self.table, self.profile, self.frontiers
        tree_id = (self.id * MAX_ITERATIONS + p.t) & M64
        nodes, todo, frontiers = [], [(int(entry_state), None, 0)], 0
        while todo:
            state, parent, slot = todo.pop()
            if len(nodes) >= MAX_NODES:
                raise Malformed(TREE)
            above = N_GAME if parent is None else parent.kind
            index = len(nodes)
            h = node_hash(self.seed, 2, tree_id, index)
            if above == N_INTERNAL:  # External(k, j): resolved, terminal
                node = Node(index, state, parent, slot, N_EXTERNAL, TERMINAL, None)
                branches = []
            elif above == N_FRONTIER:  # Internal(k): the seat opposite `internal` picks j
                node = Node(index, state, parent, slot, N_INTERNAL, self.external, self.tag + (PICK, fr.pick_info[state]))
                branches = [(state, node, j) for j in range(fr.D)]
            elif T.turn[state] == CHANCE and self.origin is not None and fr.depth[state] > self.origin:  # DepthGame::at_frontier
                if fr.pick_info[state] >= fr.n_pick or fr.payoffs(T, self.profile.bp, state) is None:
                    raise Malformed(FRONTIER)
                node = Node(index, state, parent, slot, N_FRONTIER, CHANCE, None)  # stays the chance node it was grown as
                branches = [(state, node, k) for k in range(fr.D)]
                frontiers += 1
            else:
                node = Node(index, state, parent, slot, N_GAME, T.turn[state], self.tag + (GAME, T.info[state]) if T.decision(state) else None)
                branches = [(T.kids[state][k], node, k) for k in range(len(T.kids[state]))] if T.decision(state) else []
            nodes.append(node)
            if parent is not None:
                parent.kids.append(node)
            if not branches:
                continue
            if node.turn == CHANCE:  # ExternalSampling: one branch of a chance node, uniformly
                branches = [branches[pick_uniform(h, len(branches))]]
            elif node.turn != walker:
                with np.errstate(all="ignore"):
                    w = [np.fmax(x, EPS) for x in p.sampling(node.key)]
                    u = F(u01(h) * fold(w))
                    pick, cum = 0, F(0.0)
                    for a in range(len(w) - 1):
                        cum = F(cum + w[a])
                        if pick == a and cum <= u:
                            pick = a + 1
                branches = [branches[pick]]
            todo.extend(branches)
        return nodes, frontiers

    def terminal_value(self, node, hero):
        T = self.table
        if node.kind == N_EXTERNAL:  # DepthGame::payoff: payoffs[k][j] to `internal`, negated to the other seat
            val = self.frontiers.payoffs(T, self.profile.bp, node.state)[node.parent.slot][node.slot]
            return val if hero == 1 - self.external else F(-val)
        if node.turn == TERMINAL:
            return T.payoffs[T.row[node.state] * T.n_players + hero]
        n = node.parent  # a chance leaf: cum_payoff(info, first choice) of the nearest ancestor that is not chance
        while n is not None and n.turn == CHANCE:
            n = n.parent
        return self.profile.cum(n.key, 0, "payoff")

    def recursed_value(self, root, node, rr, sr, walker):
        p = self.profile
        with np.errstate(all="ignore"):
            if not node.kids:
                return F(F(rr / sr) * self.terminal_value(node, root.turn))
            chance, sampled = node.turn == CHANCE, node.turn != CHANCE and node.turn != walker
            policy = None if chance else p.iterated(node.key)
            sampling = p.sampling(node.key) if sampled else None
            total = F(0.0)
            for child in sorted(node.kids, key=lambda k: k.slot):
                r = rr if chance else F(rr * policy[child.slot])
                s = F(sr * sampling[child.slot]) if sampled else sr
                total = F(total + self.recursed_value(root, child, r, s, walker))
            return total

    def ancestor_reach(self, root, walker):
        p = self.profile
        cf, sm = F(1.0), F(1.0)
        child, parent = root, root.parent
        with np.errstate(all="ignore"):
            while parent is not None:
                if parent.turn != walker and parent.turn != CHANCE:
                    cf = F(cf * p.iterated(parent.key)[child.slot])
                    sm = F(sm * p.sampling(parent.key)[child.slot])
                child, parent = parent, parent.parent
            return F(cf / sm)

    def dfs(self, span, walker):
        policy = self.profile.iterated(span[0].key)
        regrets, payoff = {}, F(0.0)
        with np.errstate(all="ignore"):
            for root in span:
                reach = self.ancestor_reach(root, walker)
                actions = [(c.slot, F(reach * self.recursed_value(root, c, F(1.0), F(1.0), walker))) for c in sorted(root.kids, key=lambda k: k.slot)]
                ev = fold(F(policy[a] * v) for a, v in actions)
                payoff = F(payoff + ev)
                for a, v in actions:
                    regrets[a] = F(regrets.get(a, F(0.0)) + F(v - ev))
        return regrets, payoff

    def batch(self, nodes, walker):
        """Solver::batch: the Decisions of every infoset whose head's turn is the walker, in ascending head-node order"""
        spans = {}
        for n in nodes:
            if n.key is not None and n.kids:
                spans.setdefault(n.key, []).append(n)
        updates = []
        for key, span in spans.items():
            if span[0].turn != walker:
                continue
            regret, payoff = self.dfs(span, walker)
            updates.append((key, regret, self.profile.iterated(key), payoff))
        return updates

    def apply(self, updates, row_limit):
        """update_regret, update_weight, update_payoff, update_visits per infoset (mccfr/src/solver/solver.rs:143-192)"""
        p = self.profile
        with np.errstate(all="ignore"):
            for key, regret, policy, payoff in updates:
                if row_limit is not None and key not in p.local and len(p.local) >= row_limit:
                    raise Malformed(ROWS)
                for a, delta in sorted(regret.items()):
                    total = p.cum(key, a, "regret")
                    p.mut(key, a)["regret"] = np.fmax(F(total + delta), F(-np.inf))
                for a, delta in enumerate(policy):
                    total = p.cum(key, a, "weight")
                    p.mut(key, a)["weight"] = np.fmax(F(total + F(delta * F(p.t))), EPS)
                for a in range(p.n(key)):
                    n = int(p.cum(key, a, "visits"))
                    e = p.mut(key, a)
                    e["payoff"] = F(e["payoff"] + F(F(payoff - e["payoff"]) / F(n + 1)))
                for a in range(p.n(key)):
                    p.mut(key, a)["visits"] += 1

    def exported(self, world_of_key):
        """the local profile as rows (world, kind, n_actions, id, enc[16]) in key order"""
        p, rows = self.profile, []
        for key in sorted(p.local):
            enc = np.zeros(16, ENC)
            for a, x in p.local[key].items():
                enc[a] = (x["weight"], x["regret"], x["payoff"], x["visits"])
            rows.append((world_of_key(key), key[-2], p.n(key), key[-1], enc))
        return rows


class WithOrigin(Flow, M.Solve):
    """SubGameSolver::with_origin over an entry record; origin: 0 .. 253, ORIGIN_ENTRY (depth[observed]) or ORIGIN_NONE"""

    def __init__(self, table, bp, frontiers: Frontiers, entry, origin=ORIGIN_ENTRY, index=0, hyper=None, prior=float(1 << 14), seed=0, first_id=0):
        M.Solve.__init__(self, table, bp, entry, index, hyper, prior, seed, first_id)
        self.frontiers, self.external = frontiers, int(entry["external"])
        self.profile = Profile(table, bp, hyper or M.Hyper(), prior, frontiers.D)
        origin = frontiers.depth[int(entry["observed"])] if origin == ORIGIN_ENTRY else origin
        self.origin = None if origin == ORIGIN_NONE else int(origin)
        self.counters["frontiers"] = 0
        self.tag = ()

    def step(self):
        p = self.profile
        walker = p.t % 2
        world = self.draw_world()
        self.drawn[world] += 1
        self.entry_state, chosen = self.restrict(world)
        self.counters["fallbacks"] += 0 if chosen else 1
        self.tag = (world,)
        nodes, frontiers = self.grow(self.entry_state, walker)
        self.counters["nodes"] += len(nodes)
        self.counters["frontiers"] = (self.counters["frontiers"] + frontiers) & 0xFFFFFFFF
        updates = self.batch(nodes, walker)
        self.apply(updates, min(MAX_ROWS, 4 * (self.table.n_infos + self.frontiers.n_pick)))
        self.counters["infosets"] += len(updates)
        self.trees.append(nodes)
        p.t += 1

    def harvest(self):
        T, p, e = self.table, self.profile, self.e
        out = failed(OK)
        info = int(e["harvest_info"])
        if info == NO_INFO and T.decision(self.entry_state):
            info = T.info[self.entry_state]
        if info != NO_INFO:
            n = T.actions[info]
            order = [int(x) for x in e["harvest_order"][:n]]
            if sorted(order) != list(range(n)):
                raise Malformed(M.ORDER)
            with np.errstate(all="ignore"):
                dists = [p.iterated((w, GAME, info)) for w in range(self.W)]
                for a in range(n):
                    out["refined"][a] = fold(F(dists[w][a] / F(self.W)) for w in range(self.W))
                    out["visits"][a] = sum(int(p.cum((w, GAME, info), a, "visits")) for w in range(self.W)) & 0xFFFFFFFF
                out["regret"] = fold(np.fmax(p.cum((w, GAME, info), a, "regret"), F(0.0)) for a in order for w in range(self.W))
            out["info"], out["n_actions"] = info, n
        rows = self.exported(lambda key: key[0])
        out.update(sum_regret=p.sum_regret(), iterations=p.t, n_rows=len(rows), rows=rows, drawn=self.drawn.copy(), **self.counters)
        return out


class DepthSolver(Flow):
    """DepthSolver::new(source, prefix, internal, entry) — the prefix is in the table's infoset ids — with step and harvest"""

    def __init__(self, table, bp, frontiers: Frontiers, state, internal, index=0, hyper=None, prior=float(1 << 14), seed=0, first_id=0):
        self.table, self.frontiers, self.seed, self.id = table, frontiers, seed, (first_id + index) & M64
        self.profile = Profile(table, bp, hyper or M.Hyper(), prior, frontiers.D)
        self.entry, self.external, self.tag = int(state), 1 - internal, ()
        self.origin = frontiers.depth[self.entry]  # Some(entry.depth())
        self.nodes = self.infosets = self.n_frontiers = 0

    def step(self):
        walker = self.profile.t % 2
        nodes, frontiers = self.grow(self.entry, walker)
        updates = self.batch(nodes, walker)
        self.apply(updates, None)
        self.nodes, self.infosets, self.n_frontiers = self.nodes + len(nodes), self.infosets + len(updates), self.n_frontiers + frontiers
        self.profile.t += 1  # advance

    def harvest(self, info, order):
        """Harvest::harvest(base): refined, visits, regret over the Game edges of `info`, the edges in `order` (E's derived Ord)"""
        p, key = self.profile, (GAME, info)
        with np.errstate(all="ignore"):
            refined = p.iterated(key)
            visits = [int(p.cum(key, a, "visits")) for a in range(p.n(key))]
            regret = fold(np.fmax(p.cum(key, a, "regret"), F(0.0)) for a in order[:p.n(key)])
        return refined, visits, regret


def failed(status):
    out = M.failed(status)
    out["frontiers"] = 0
    return out


def solve(table, bp, frontiers, entry, origin=ORIGIN_ENTRY, index=0, iterations=1, keep=None, **kw):
    """one entry (a SUBGAME_ENTRY_DTYPE record) of a batch -> harvest dict; a malformed entry answers zeros and its status"""
    try:
        s = WithOrigin(table, bp, frontiers, entry, origin, index, **kw)
        if keep is not None:
            keep.append(s)
        for _ in range(iterations):
            s.step()
        return s.harvest()
    except Malformed as m:
        return failed(m.status)


def compare(result, rows, model, rows_cap):
    """asserts a device result record (SUBGAME_RESULT_DTYPE) and its rows (SUBGAME_ROW_DTYPE [rows_cap]) equal the model's bit for bit"""
    for f in ("status", "info", "n_actions", "iterations", "n_rows", "nodes", "infosets", "fallbacks", "frontiers"):
        assert int(result[f]) == int(model[f]), (f, int(result[f]), int(model[f]))
    assert np.array_equal(result["drawn"], model["drawn"]), (result["drawn"], model["drawn"])
    assert np.array_equal(result["visits"], model["visits"])
    assert np.array_equal(result["refined"].view(np.uint32), model["refined"].view(np.uint32)), (result["refined"], model["refined"])
    for f in ("regret", "sum_regret"):
        assert F(result[f]).view(np.uint32) == F(model[f]).view(np.uint32), (f, result[f], model[f])
    for i in range(rows_cap):
        if i < len(model["rows"]):
            world, kind, n, info, enc = model["rows"][i]
            got = (int(rows[i]["world"]), int(rows[i]["kind"]), int(rows[i]["n_actions"]), int(rows[i]["info"]))
            assert got == (world, kind, n, info), (i, got, (world, kind, n, info))
            assert rows[i]["enc"].tobytes() == enc.tobytes(), (i, rows[i]["enc"][:n], enc[:n])
        else:
            assert not rows[i].tobytes().strip(b"\0"), f"row {i} past n_rows is not zero"

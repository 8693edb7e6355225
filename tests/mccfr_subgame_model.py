"""The model the table-game subgame tests compare against (helper, no tests): rp_mccfr_subgame_belief and rp_mccfr_subgame_solve
(include/rp_mi355x.h) by the NAIVE algorithm of the reference's text — Posterior::add and Partition::partition::<W>
(subgame/src/world/partition.rs:26-52), Solver::external_reach (mccfr/src/solver/solver.rs:198-210), the encoders' `restrict`
(kuhn/src/encoder.rs:47-66, leduc/src/encoder.rs:48-68) with Belief::remember, SubGameSolver::step / Harvest::harvest with origin =
None (subgame/src/solver.rs:146-229), WorldEncoder::branches (world/encoder.rs:100-107), TreeBuilder with ExternalSampling
(mccfr/src/solver/builder.rs, sample/external.rs), Tree::partition, CfrFlow::dfs / recursed_value / ancestor_reach (strategy/flow.rs),
CfrNash::terminal_value (strategy/nash.rs:50-79), the warmstart (strategy/profile.rs:94-104) and the four Solver::update_*
(solver/solver.rs:143-192).

Everything is spelt out: np.float32 scalars with one rounding per operation, sequential folds, recursion for the values, the local
profile as a dict (world, info) -> slot -> Encounter created edge by edge from `warmstart`.  A game is read through the ctypes
rp_game_table, a blueprint as Solver.export returns it.  The kernel (robopoker_amd/csrc/mccfr_subgame.hpp) keeps whole rows in a
region, an index instead of a dict and level-by-level sweeps instead of the recursion, so that this checks them."""
from __future__ import annotations

import numpy as np

from robopoker_amd import _lib

F = np.float32
EPS = F(1.17549435e-38)
M64 = (1 << 64) - 1
CHANCE, TERMINAL, NO_INFO, WORLD_NONE = _lib.RP_TURN_CHANCE, _lib.RP_TURN_TERMINAL, _lib.RP_NO_INFO, _lib.RP_WORLD_NONE
MAX_ITERATIONS, MAX_NODES, MAX_ROWS = 1 << 20, 62, 1024
(OK, SEAT, MODE, WORLDS, COUNT, STATE, SECRET, PATH, WEIGHT, INFO, TREE, ROWS, ORDER) = range(13)
ENC = np.dtype([("weight", "<f4"), ("regret", "<f4"), ("payoff", "<f4"), ("visits", "<u4")])


class Malformed(Exception):
    def __init__(self, status):
        super().__init__(status)
        self.status = status


# ---- include/rp_math.h, restated ----
def _mix64(z):
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _fmix32(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def node_hash(seed, epoch, tree, key):
    h = _mix64((seed + 0x9E3779B97F4A7C15) & M64)
    h = _mix64(h ^ ((epoch * 0xD1342543DE82EF95 + 0x632BE59BD9B4E019) & M64))
    h = _mix64(h ^ ((tree * 0xAF251AF3B0F025B5 + 0x2545F4914F6CDD1D) & M64))
    k = (key ^ (key >> 32)) & 0xFFFFFFFF
    x = _fmix32((h & 0xFFFFFFFF) ^ k)
    x = ((x ^ (h >> 32)) * 0x9E3779B1) & 0xFFFFFFFF
    x ^= x >> 15
    return x << 32


def u01(h):
    return F(F(h >> 40) * F(5.9604644775390625e-8))


def fold(xs):
    total = F(0.0)
    for x in xs:
        total = F(total + x)
    return total


class Hyper:
    def __init__(self, temperature=1.0, smoothing=2.0, curiosity=0.05):
        self.temperature, self.smoothing, self.curiosity = F(temperature), F(smoothing), F(curiosity)


# ---- the game and the blueprint ----
class Table:
    """an rp_game_table (ctypes) as python lists"""

    def __init__(self, t):
        self.n_states, self.n_infos, self.n_players, self.A, self.n_terminals = t.n_states, t.n_infos, t.n_players, t.max_actions, t.n_terminals
        self.turn = [t.states[s].turn for s in range(t.n_states)]
        self.info = [t.states[s].info for s in range(t.n_states)]
        self.kids = [[t.children[t.states[s].offset + k] for k in range(t.states[s].n_children)] for s in range(t.n_states)]
        self.row = [t.states[s].offset for s in range(t.n_states)]
        self.payoffs = [F(t.payoffs[i]) for i in range(t.n_terminals * t.n_players)]
        self.actions = [t.info_actions[i] for i in range(t.n_infos)]

    def decision(self, s):
        return self.turn[s] < self.n_players and len(self.kids[s]) > 0


class Blueprint:
    """Solver.export()'s rows, [n_infos * A] of ENC"""

    def __init__(self, table: Table, rows):
        self.rows = np.asarray(rows, dtype=ENC).reshape(table.n_infos, table.A)

    def get(self, info, a, field):
        return self.rows[info, a][field]

    def averaged(self, info, n):
        with np.errstate(all="ignore"):
            w = [np.fmax(self.get(info, a, "weight"), EPS) for a in range(n)]
            total = fold(w)
            return [F(x / total) for x in w]


# ---- BELIEF ----
def partition(entries, W):
    """entries: [(secret, mass)] in ascending secret -> ({secret: world}, weights[4]); Partition::partition::<W>"""
    weights = np.zeros(4, F)
    with np.errstate(all="ignore"):
        total = fold(m for _, m in entries)
        if not total > 0:
            weights[:W] = F(F(1.0) / F(W))
            return {s: 0 for s, _ in entries}, weights
        ordered = []  # sort_by(b.partial_cmp(a)), stable: an entry passes only strictly smaller masses
        for s, m in entries:
            at = len(ordered)
            while at > 0 and ordered[at - 1][1] < m:
                at -= 1
            ordered.insert(at, (s, m))
        segment = F(total / F(W))
        mapping, index, bucket, accumulated = {}, 0, F(0.0), F(0.0)
        for s, m in ordered:
            bucket = F(bucket + m)
            accumulated = F(accumulated + m)
            mapping[s] = index
            if accumulated >= F(segment * F(index + 1)) and index < W - 1:
                weights[index] = F(bucket / total)
                index += 1
                bucket = F(0.0)
        weights[index] = F(bucket / total)
        return mapping, weights


def belief(table: Table, bp: Blueprint, prior) -> dict:
    """one SUBGAME_PRIOR_DTYPE record -> {"world_of" [16] u8, "weights" [4] f32, "status"}"""
    out = {"world_of": np.full(16, WORLD_NONE, np.uint8), "weights": np.zeros(4, F), "status": OK}
    try:
        n, n_path, W = int(prior["n_prior"]), int(prior["n_path"]), int(prior["n_worlds"])
        internal, mode = int(prior["internal"]), int(prior["mode"])
        if internal > 1:
            raise Malformed(SEAT)
        if mode > 1:
            raise Malformed(MODE)
        if not 1 <= W <= 4:
            raise Malformed(WORLDS)
        if n > 16 or n_path > 16:
            raise Malformed(COUNT)
        posterior = {}
        for c in range(n):
            secret, s = int(prior["secret"][c]), int(prior["root_state"][c])
            if secret >= 16:
                raise Malformed(SECRET)
            if s >= table.n_states:
                raise Malformed(STATE)
            mass = F(1.0)
            for k in range(n_path):
                slot = int(prior["path"][k])
                if slot >= len(table.kids[s]):
                    raise Malformed(PATH)
                if mode == 1 and table.turn[s] == 1 - internal:  # is_opponent(hero): averaged_policy(info, edge)
                    mass = F(mass * bp.averaged(table.info[s], table.actions[table.info[s]])[slot])
                s = table.kids[s][slot]
            posterior[secret] = F(posterior.get(secret, F(0.0)) + mass)  # Posterior::add
        mapping, weights = partition(sorted(posterior.items()), W)
        for s, w in mapping.items():
            out["world_of"][s] = w
        out["weights"] = weights
    except Malformed as m:
        out["status"] = m.status
    return out


# ---- WorldProfile over the blueprint ----
class Profile:
    def __init__(self, table, bp, hyper, prior):
        self.table, self.bp, self.hp, self.prior, self.local, self.t = table, bp, hyper, F(prior), {}, 0

    def n(self, key):
        return self.table.actions[key[1]]

    def cum(self, key, a, field):
        e = self.local.get(key, {}).get(a)
        if e is not None:
            return e[field]
        v = self.bp.get(key[1], a, field)
        return np.fmax(v, EPS) if field in ("weight", "regret") else v

    def mut(self, key, a):
        edges = self.local.setdefault(key, {})
        if a not in edges:  # warmstart from the untagged blueprint row; its regret is overwritten by the update that creates the edge
            k = self.prior
            with np.errstate(all="ignore"):
                p = self.bp.averaged(key[1], self.n(key))[a]
                edges[a] = {"weight": F(F(F(p * k) * F(k + F(1.0))) / F(2.0)), "regret": F(0.0), "payoff": F(0.0), "visits": 0}
        return edges[a]

    def regret(self, key, a):
        return np.fmax(self.cum(key, a, "regret"), EPS)

    def weight(self, key, a):
        return np.fmax(self.cum(key, a, "weight"), EPS)

    def iterated(self, key):
        with np.errstate(all="ignore"):
            r = [np.fmax(self.regret(key, a), EPS) for a in range(self.n(key))]
            total = fold(r)
            return [F(x / total) for x in r]

    def sampling(self, key):
        hp = self.hp
        with np.errstate(all="ignore"):
            w = [np.fmax(self.weight(key, a), EPS) for a in range(self.n(key))]
            denom = F(fold(w) + hp.smoothing)
            raw = [np.fmax(F(F(F(x / hp.temperature) + hp.smoothing) / denom), hp.curiosity) for x in w]
            z = fold(raw)
            return [F(x / z) for x in raw]

    def sum_regret(self):
        total = fold(np.fmax(self.local[key][a]["regret"], F(0.0)) for key in sorted(self.local) for a in sorted(self.local[key]))
        return F(total / F(max(self.t, 1)))


class Node:
    def __init__(self, index, state, parent, slot):
        self.index, self.state, self.parent, self.slot, self.kids = index, state, parent, slot, []


class Solve:
    def __init__(self, table: Table, bp: Blueprint, entry, index=0, hyper=None, prior=float(1 << 14), seed=0, first_id=0):
        self.table, self.e, self.seed = table, entry, seed
        self.id = (first_id + index) & M64
        self.profile = Profile(table, bp, hyper or Hyper(), prior)
        e = entry
        self.W, self.n_cand = int(e["n_worlds"]), int(e["n_candidates"])
        if int(e["external"]) > 1:
            raise Malformed(SEAT)
        if not 1 <= self.W <= 4:
            raise Malformed(WORLDS)
        if self.n_cand > 16:
            raise Malformed(COUNT)
        if int(e["observed"]) >= table.n_states or any(int(c) >= table.n_states for c in e["candidate"][:self.n_cand]):
            raise Malformed(STATE)
        if any(int(s) >= 16 for s in e["secret"][:self.n_cand]):
            raise Malformed(SECRET)
        if any(not (x >= 0) or np.isinf(x) for x in e["weights"][:self.W]):
            raise Malformed(WEIGHT)
        if int(e["harvest_info"]) != NO_INFO and int(e["harvest_info"]) >= table.n_infos:
            raise Malformed(INFO)
        self.world_of = [int(w) if int(w) < self.W else WORLD_NONE for w in e["world_of"]]
        self.counters = {"nodes": 0, "infosets": 0, "fallbacks": 0}
        self.drawn = np.zeros(4, np.uint32)
        self.entry_state, self.trees = None, []

    def draw_world(self):
        w = [F(x) for x in self.e["weights"][:self.W]]
        x = F(u01(node_hash(self.seed, 1, self.id, self.profile.t)) * fold(w))
        run = F(0.0)
        for i, wi in enumerate(w):
            run = F(run + wi)
            if x < run:
                return i
        nonzero = [i for i, wi in enumerate(w) if wi != 0]
        return nonzero[-1] if nonzero else 0

    def restrict(self, world):
        """-> (state, whether a candidate was chosen)"""
        empty = all(w == WORLD_NONE for w in self.world_of)
        for c in range(self.n_cand):
            if empty or self.world_of[int(self.e["secret"][c])] == world:
                return int(self.e["candidate"][c]), True
        return int(self.e["observed"]), False

    def build(self, world, walker):
        T, p = self.table, self.profile
        tree_id = (self.id * MAX_ITERATIONS + p.t) & M64
        nodes, todo = [], [(int(self.entry_state), None, 0)]
        while todo:
            state, parent, slot = todo.pop()
            if len(nodes) >= MAX_NODES:
                raise Malformed(TREE)
            node = Node(len(nodes), state, parent, slot)
            nodes.append(node)
            if parent is not None:
                parent.kids.append(node)
            if not T.decision(state):
                continue
            branches = [(T.kids[state][k], node, k) for k in range(len(T.kids[state]))]
            if T.turn[state] != walker:
                with np.errstate(all="ignore"):
                    w = [np.fmax(x, EPS) for x in p.sampling((world, T.info[state]))]
                    u = F(u01(node_hash(self.seed, 2, tree_id, node.index)) * fold(w))
                    pick, cum = 0, F(0.0)
                    for a in range(len(w) - 1):
                        cum = F(cum + w[a])
                        if pick == a and cum <= u:
                            pick = a + 1
                branches = [branches[pick]]
            todo.extend(branches)
        return nodes

    def terminal_value(self, node, hero, world):
        T = self.table
        if T.turn[node.state] == TERMINAL:
            return T.payoffs[T.row[node.state] * T.n_players + hero]
        # a chance leaf (rp_game_table_check refuses a player state without children, so a leaf is terminal or chance): the nearest
        # ancestor that is not chance
        n = node.parent
        while n is not None and T.turn[n.state] == CHANCE:
            n = n.parent
        return self.profile.cum((world, T.info[n.state]), 0, "payoff")

    def recursed_value(self, root, node, rr, sr, walker, world):
        T, p = self.table, self.profile
        with np.errstate(all="ignore"):
            if not node.kids:
                return F(F(rr / sr) * self.terminal_value(node, T.turn[root.state], world))
            key = (world, T.info[node.state])
            sampled = T.turn[node.state] != walker
            policy, sampling = p.iterated(key), (p.sampling(key) if sampled else None)
            total = F(0.0)
            for child in sorted(node.kids, key=lambda k: k.slot):
                r = F(rr * policy[child.slot])
                s = F(sr * sampling[child.slot]) if sampled else sr
                total = F(total + self.recursed_value(root, child, r, s, walker, world))
            return total

    def ancestor_reach(self, root, walker, world):
        T, p = self.table, self.profile
        cf, sm = F(1.0), F(1.0)
        child, parent = root, root.parent
        with np.errstate(all="ignore"):
            while parent is not None:
                if T.turn[parent.state] != walker:
                    key = (world, T.info[parent.state])
                    cf = F(cf * p.iterated(key)[child.slot])
                    sm = F(sm * p.sampling(key)[child.slot])
                child, parent = parent, parent.parent
            return F(cf / sm)

    def dfs(self, span, walker, world):
        T, p = self.table, self.profile
        key = (world, T.info[span[0].state])
        policy = p.iterated(key)
        regrets, payoff = {}, F(0.0)
        with np.errstate(all="ignore"):
            for root in span:
                reach = self.ancestor_reach(root, walker, world)
                actions = [(c.slot, F(reach * self.recursed_value(root, c, F(1.0), F(1.0), walker, world))) for c in sorted(root.kids, key=lambda k: k.slot)]
                ev = fold(F(policy[a] * v) for a, v in actions)
                payoff = F(payoff + ev)
                for a, v in actions:
                    regrets[a] = F(regrets.get(a, F(0.0)) + F(v - ev))
        return regrets, payoff

    def step(self):
        T, p = self.table, self.profile
        walker = p.t % 2
        world = self.draw_world()
        self.drawn[world] += 1
        self.entry_state, chosen = self.restrict(world)
        self.counters["fallbacks"] += 0 if chosen else 1
        nodes = self.build(world, walker)
        self.counters["nodes"] += len(nodes)
        spans = {}
        for n in nodes:
            if n.kids:
                spans.setdefault((world, T.info[n.state]), []).append(n)
        updates = []
        for key, span in spans.items():  # ascending head-node order
            if T.turn[span[0].state] != walker:
                continue
            regret, payoff = self.dfs(span, walker, world)
            updates.append((key, regret, p.iterated(key), payoff))
        with np.errstate(all="ignore"):
            for key, regret, policy, payoff in updates:
                if key not in p.local and len(p.local) >= min(MAX_ROWS, 4 * T.n_infos):
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
                raise Malformed(ORDER)
            with np.errstate(all="ignore"):
                dists = [p.iterated((w, info)) for w in range(self.W)]
                for a in range(n):
                    out["refined"][a] = fold(F(dists[w][a] / F(self.W)) for w in range(self.W))
                    out["visits"][a] = sum(int(p.cum((w, info), a, "visits")) for w in range(self.W)) & 0xFFFFFFFF
                out["regret"] = fold(np.fmax(p.cum((w, info), a, "regret"), F(0.0)) for a in order for w in range(self.W))
            out["info"], out["n_actions"] = info, n
        rows = []
        for key in sorted(p.local):
            enc = np.zeros(16, ENC)
            for a, x in p.local[key].items():
                enc[a] = (x["weight"], x["regret"], x["payoff"], x["visits"])
            rows.append((key[0], p.n(key), key[1], enc))
        out.update(sum_regret=p.sum_regret(), iterations=p.t, n_rows=len(rows), rows=rows, drawn=self.drawn.copy(), **self.counters)
        return out


def failed(status):
    return {"status": status, "info": NO_INFO, "n_actions": 0, "refined": np.zeros(16, F), "visits": np.zeros(16, np.uint32), "regret": F(0.0),
            "sum_regret": F(0.0), "iterations": 0, "n_rows": 0, "nodes": 0, "infosets": 0, "drawn": np.zeros(4, np.uint32), "fallbacks": 0,
            "rows": []}


def solve(table, bp, entry, index=0, iterations=1, keep=None, **kw):
    """one entry (a SUBGAME_ENTRY_DTYPE record) of a batch -> harvest dict; a malformed entry answers zeros and its status"""
    try:
        s = Solve(table, bp, entry, index, **kw)
        if keep is not None:
            keep.append(s)
        for _ in range(iterations):
            s.step()
        return s.harvest()
    except Malformed as m:
        return failed(m.status)


def averaged_policy(table, bp, result_rows, info, n_worlds):
    """`subpolicy` of the reference's tests (kuhn/src/solver.rs:294-310): CfrNash::averaged_policy at (world, info) — the local row's
    weights, else max(blueprint, EPSILON) — averaged over the worlds; result_rows: [(world, n_actions, info, enc)]"""
    n = table.actions[info]
    local = {(w, i): enc for w, _, i, enc in result_rows}
    out = np.zeros(n, np.float64)
    for w in range(n_worlds):
        enc = local.get((w, info))
        weights = [np.fmax(F(enc[a]["weight"]) if enc is not None else np.fmax(bp.get(info, a, "weight"), EPS), EPS) for a in range(n)]
        total = fold(weights)
        out += np.array([F(x / total) for x in weights], np.float64)
    return out / n_worlds


def compare(result, rows, model, rows_cap):
    """asserts a device result record (SUBGAME_RESULT_DTYPE) and its rows (SUBGAME_ROW_DTYPE [rows_cap]) equal the model's bit for bit"""
    for f in ("status", "info", "n_actions", "iterations", "n_rows", "nodes", "infosets", "fallbacks"):
        assert int(result[f]) == int(model[f]), (f, int(result[f]), int(model[f]))
    assert np.array_equal(result["drawn"], model["drawn"]), (result["drawn"], model["drawn"])
    assert np.array_equal(result["visits"], model["visits"])
    for f in ("refined",):
        assert np.array_equal(result[f].view(np.uint32), model[f].view(np.uint32)), (f, result[f], model[f])
    for f in ("regret", "sum_regret"):
        assert F(result[f]).view(np.uint32) == F(model[f]).view(np.uint32), (f, result[f], model[f])
    for i in range(rows_cap):
        if i < len(model["rows"]):
            world, n, info, enc = model["rows"][i]
            assert (int(rows[i]["world"]), int(rows[i]["n_actions"]), int(rows[i]["info"])) == (world, n, info)
            assert rows[i]["enc"].tobytes() == enc.tobytes(), (i, rows[i]["enc"][:n], enc[:n])
        else:
            assert not rows[i].tobytes().strip(b"\0"), f"row {i} past n_rows is not zero"

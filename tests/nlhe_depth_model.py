"""The model the depth-solver tests compare against (helper, no tests): rp_nlhe_depth_solve (include/rp_mi355x.h) by the NAIVE algorithm
of the reference — DepthSolver::step / harvest (subgame/src/depth/solver.rs:76-123) over DepthEncoder / DepthGame / DepthProfile /
DepthView (subgame/src/depth/), TreeBuilder with ExternalSampling (mccfr/src/solver/builder.rs, sample/external.rs), Tree::partition,
CfrFlow::dfs / recursed_value / ancestor_reach (strategy/flow.rs), CfrNash::terminal_value (strategy/nash.rs:50-79) and the four
Solver::update_* (solver/solver.rs:143-192).

Everything is spelt out: an explicit node list with a copy of the game per node, the todo stack of the builder, `partition` as a dict,
dfs / recursed_value as recursion over np.float32 scalars (one rounding per operation), the local profile as a dict of dicts (info ->
slot -> Encounter) that creates an edge from `warmstart` on its first write, over a blueprint that answers `get(key)` (the weights, for
the rollouts) and `enc(key)` (the whole row).  Frontier payoffs come from nlhe_rollout_model.payoffs with the id the header states.  The
kernel (robopoker_amd/csrc/nlmc_depth.hpp) keeps rows instead of edges, packed games, sibling links and two linear sweeps instead of the
recursion, so that this checks them."""
from __future__ import annotations

import ctypes as C

import numpy as np

import nlhe_policy_model as PM
import nlhe_rollout_model as FM
import oracle_nlhe as ON
from robopoker_amd.nlhe import Frontier

F = np.float32
EPS = PM.EPSILON
M64 = PM.M64
A = PM.A
MAX_ITERATIONS, MAX_FRONTIERS, MAX_NODES, MAX_INFOS, MAX_ROWS = 4096, 32, 384, 96, 512  # RP_NLHE_DEPTH_*: the header's
OK = FM.OK
NODES, ROWS, FRONTIERS = 8, 9, 10  # RP_DEPTH_NODES, RP_DEPTH_ROWS, RP_DEPTH_FRONTIERS
GAME, PICK = 0, 1
DRAW_EPOCH = 2  # the stream of the tree's own draws: the frontier rollouts use epoch 0, the worlds epoch 1
Malformed = FM.Malformed


class Hyper:
    def __init__(self, temperature=1.0, smoothing=2.0, curiosity=0.05):
        self.temperature, self.smoothing, self.curiosity = temperature, smoothing, curiosity


def fold(xs):
    total = F(0.0)
    for x in xs:
        total = F(total + x)
    return total


# ---- DepthProfile over DepthView over the blueprint ----
class Profile:
    """info = (kind, past, present, choices); an edge is its slot among info's choices"""

    def __init__(self, bp, hyper: Hyper, prior, bp_epoch: int):
        self.bp, self.hp, self.prior, self.bp_epoch, self.local, self.t = bp, hyper, F(prior), bp_epoch, {}, 0
        self.seen = []  # (info, found in the blueprint) of every view read

    @staticmethod
    def n(info) -> int:
        return 4 if info[0] == PICK else PM.nch(info[3])

    # DepthView: the blueprint, or the constants of a Pick edge
    def view(self, info, a: int, field: str):
        if info[0] == PICK:
            return {"weight": F(0.25), "regret": EPS, "payoff": F(0.0), "visits": 0}[field]
        row = self.bp.enc(info[1:])
        self.seen.append((info, row is not None))
        if row is None:  # the table's defaults, as rp_nlhe_memory reads an absent infoset
            edge = int(PM.edges(info[3])[a])
            return {"weight": F(0.0), "regret": PM.default_regret(edge), "payoff": F(0.0), "visits": 0}[field]
        return row[field][a]

    def view_warmstart(self, info, a: int):
        if info[0] == PICK:
            return {"weight": F(0.0), "regret": F(0.0), "payoff": F(0.0), "visits": 0}  # Encounter::default()
        with np.errstate(all="ignore"):
            k = self.prior
            n = self.n(info)
            policy = PM.distribution("averaged", [self.view(info, b, "weight") for b in range(n)] + [0] * (A - n), n)[a]
            scale = F(k / F(max(self.bp_epoch, 1)))
            return {"weight": F(F(F(policy * k) * F(k + F(1.0))) / F(2.0)), "regret": F(self.view(info, a, "regret") * scale),
                    "payoff": F(0.0), "visits": 0}

    def cum(self, info, a: int, field: str):
        e = self.local.get(info, {}).get(a)
        if e is not None:
            return e[field]
        v = self.view(info, a, field)
        return np.fmax(v, EPS) if field in ("weight", "regret") else v

    def mut(self, info, a: int):
        edges = self.local.setdefault(info, {})
        if a not in edges:
            edges[a] = self.view_warmstart(info, a)
        return edges[a]

    def regret(self, info, a):
        return np.fmax(self.cum(info, a, "regret"), EPS)

    def weight(self, info, a):
        return np.fmax(self.cum(info, a, "weight"), EPS)

    def regret_denom(self, info):
        return fold(self.regret(info, a) for a in range(self.n(info)))

    def iterated(self, info):
        n = self.n(info)
        return PM.distribution("iterated", [self.regret(info, a) for a in range(n)] + [0] * (A - n), n)[:n]

    def sampling(self, info):
        n = self.n(info)
        return PM.distribution("sampling", [self.weight(info, a) for a in range(n)] + [0] * (A - n), n, self.hp.temperature,
                               self.hp.smoothing, self.hp.curiosity)[:n]

    def instant_policy(self, info, a):
        with np.errstate(all="ignore"):
            return F(self.regret(info, a) / self.regret_denom(info))

    def frontier_payoff(self, info):
        return self.cum(info, 0, "payoff")

    def sorted_infos(self):
        return sorted(self.local)

    def sum_regret(self):
        """the reference folds a HashMap; the library states the order: rows ascending, slots ascending"""
        total = fold(np.fmax(self.local[info][a]["regret"], F(0.0)) for info in self.sorted_infos() for a in sorted(self.local[info]))
        return F(total / F(max(self.t, 1)))


# ---- the tree ----
class Node:
    def __init__(self, index, game, story, parent, edge, phase, k=0, j=0):
        self.index, self.game, self.story, self.parent, self.edge, self.phase, self.k, self.j = index, game, story, parent, edge, phase, k, j
        self.kids, self.info, self.frontier, self.payoffs = [], None, None, None

    def edges(self):
        """Node::edges: petgraph walks a node's outgoing edges newest first"""
        return list(reversed(self.kids))


def inner_turn(g) -> int:
    return ON.lib().ora_nlhe_turn(C.byref(g))


def street(g) -> int:
    return ON.lib().ora_nlhe_street(C.byref(g))


class Solve:
    """one solve: entry = a Frontier record (its `internal` the seat solved for), origin = the depth the frontier lies beyond"""

    def __init__(self, entry, origin, bp, index=0, hyper=None, bp_epoch=0, rollouts=16, bias=5.0, prior=float(1 << 14), seed=0, first_id=0):
        self.entry, self.origin, self.bp, self.rollouts, self.bias, self.seed = entry, origin, bp, max(rollouts, 1), bias, seed
        self.id = (first_id + index) & M64
        self.profile = Profile(bp, hyper or Hyper(), prior, bp_epoch)
        self.game = FM.frontier_game(entry)  # validates; raises Malformed
        self.internal = entry.internal
        self.counters = {"nodes": 0, "infosets": 0, "frontiers": 0, "rollouts": 0}
        self.trees, self.spans, self.frontier_log = [], [], []  # kept for the tests: the last tree, (walker, info, span) and payoffs

    # DepthGame
    def turn(self, node) -> int:
        if node.phase == "D":
            return inner_turn(node.game)
        return 1 - self.internal if node.phase == "I" else ON.TERMINAL

    def at_frontier(self, node) -> bool:
        return node.phase == "D" and inner_turn(node.game) == ON.CHANCE and street(node.game) > self.origin

    def key(self, node):
        g = node.game
        actor = inner_turn(g) if inner_turn(g) >= 0 else (g.dealer + g.ticker) % 2  # sweat() reads the ticker's seat
        return FM.key_at(g, list(self.entry.prefix) + node.story, actor)

    # DepthEncoder::branches: [(edge, phase, k, j, game, story)]
    def branches(self, node):
        if self.at_frontier(node) or node.phase == "I":
            nxt = "I" if node.phase == "D" else "E"
            return [(c, nxt, c if nxt == "I" else node.k, c if nxt == "E" else 0, node.game, node.story) for c in range(4)]
        if node.phase == "E" or inner_turn(node.game) < 0:
            return []
        o, out = ON.lib(), []
        edges = PM.edges(node.info[3])[:PM.nch(node.info[3])]
        if len(edges) == 0:
            raise Malformed(FM.ILLEGAL)
        for e in edges:
            g = FM._copy(node.game)
            action = o.ora_nlhe_snap(C.byref(g), o.ora_nlhe_actionize(C.byref(g), int(e), 0))
            if o.ora_nlhe_apply(C.byref(g), C.byref(action)):
                raise Malformed(FM.ILLEGAL)
            out.append((int(e), "D", 0, 0, g, node.story + [int(e)]))
        return out

    def info_of(self, node):
        if node.phase == "I":  # the chance node's NlheInfo: its choices are the one-edge Path [Draw] (game.choices at a chance node)
            return (PICK,) + self.key(node)[:2] + (ON.E_DRAW,)
        if node.phase == "D" and inner_turn(node.game) >= 0:
            return (GAME,) + self.key(node)
        return None  # a chance or terminal node: its info is never read

    def tree_id(self) -> int:
        return (self.id * MAX_ITERATIONS + self.profile.t) & M64

    # ExternalSampling::sample
    def sample(self, node, branches, walker):
        if not branches:
            return branches
        turn = self.turn(node)
        if turn == walker:
            return branches
        h = FM.node_hash(self.seed, DRAW_EPOCH, self.tree_id(), node.index)
        if turn == ON.CHANCE:  # randomly: the frontier node is still the chance node it was grown as
            return [branches[FM.pick_uniform(h, len(branches))]]
        with np.errstate(all="ignore"):
            w = [np.fmax(x, EPS) for x in self.profile.sampling(node.info)]
            total = fold(w)
            u = F(FM.u01(h) * total)
            pick, cum = 0, F(0.0)
            for a in range(len(w) - 1):
                cum = F(cum + w[a])
                if pick == a and cum <= u:
                    pick = a + 1
        return [branches[pick]]

    def grow(self, nodes, leaf, frontiers):
        edge, phase, k, j, game, story, parent = leaf
        if len(nodes) >= MAX_NODES:
            raise Malformed(NODES)
        node = Node(len(nodes), game, story, parent, edge, phase, k, j)
        nodes.append(node)
        if parent is not None:
            parent.kids.append(node)
        node.info = self.info_of(node)
        if self.at_frontier(node):
            if len(frontiers) >= MAX_FRONTIERS:
                raise Malformed(FRONTIERS)
            node.frontier = len(frontiers)
            frontiers.append(node)
        return node

    def build(self, walker):
        nodes, frontiers, todo = [], [], []
        root = self.grow(nodes, (None, "D", 0, 0, self.game, [], None), frontiers)
        todo.extend(b + (root,) for b in self.sample(root, self.branches(root), walker))
        while todo:
            node = self.grow(nodes, todo.pop(), frontiers)
            todo.extend(b + (node,) for b in self.sample(node, self.branches(node), walker))
        return nodes, frontiers

    def frontier_payoffs(self, node):
        f = self.entry
        record = Frontier(f.holes, f.internal, f.draws, tuple(f.edges) + tuple(node.story), f.prefix, f.stacks, f.dealer)
        fid = ((self.tree_id() * MAX_FRONTIERS) + node.frontier) & M64
        status, pay, _ = FM.payoffs(record, self.bp, 0, self.bias, self.rollouts, self.seed, fid)
        if status != OK:
            raise Malformed(status)
        self.frontier_log.append((record, fid, pay))
        return pay

    # CfrNash::terminal_value
    def terminal_value(self, node, hero):
        turn = self.turn(node)
        if turn == ON.TERMINAL:
            if node.phase == "E":
                n = node
                while n.frontier is None:
                    n = n.parent
                val = n.payoffs[node.k, node.j]
                return val if hero == self.internal else F(-val)
            out = C.c_float()
            assert ON.lib().ora_nlhe_payoff(C.byref(node.game), hero, C.byref(out)) == 0
            return F(out.value)
        assert turn == ON.CHANCE  # a decision node always has choices
        n = node.parent
        while self.turn(n) == ON.CHANCE:
            n = n.parent
        return self.profile.frontier_payoff(n.info)

    def recursed_value(self, root, node, rr, sr, walker):
        p = self.profile
        with np.errstate(all="ignore"):
            if not node.kids:
                return F(F(rr / sr) * self.terminal_value(node, self.turn(root)))
            turn = self.turn(node)
            chance = turn == ON.CHANCE
            sampled = not chance and turn != walker
            sampling = p.sampling(node.info) if sampled else None
            total = F(0.0)
            for child in node.edges():
                a = self.slot(node, child)
                r = rr if chance else F(rr * p.instant_policy(node.info, a))
                s = F(sr * sampling[a]) if sampled else sr
                total = F(total + self.recursed_value(root, child, r, s, walker))
            return total

    @staticmethod
    def slot(node, child) -> int:
        if node.phase == "I" or node.frontier is not None:
            return child.edge
        return list(PM.edges(node.info[3])).index(child.edge)

    def ancestor_reach(self, root, walker):
        p = self.profile
        cf, sm = F(1.0), F(1.0)
        child, parent = root, root.parent
        with np.errstate(all="ignore"):
            while parent is not None:
                turn = self.turn(parent)
                if turn != ON.CHANCE and turn != walker:
                    a = self.slot(parent, child)
                    cf = F(cf * p.instant_policy(parent.info, a))
                    sm = F(sm * p.sampling(parent.info)[a])
                child, parent = parent, parent.parent
            return F(cf / sm)

    def dfs(self, span, walker):
        p = self.profile
        info = span[0].info
        with np.errstate(all="ignore"):
            rd = p.regret_denom(info)
            regrets, payoff = {}, F(0.0)
            for root in span:
                reach = self.ancestor_reach(root, walker)
                actions = [(self.slot(root, c), F(reach * self.recursed_value(root, c, F(1.0), F(1.0), walker))) for c in root.edges()]
                ev = fold(F(F(p.regret(root.info, a) / rd) * v) for a, v in actions)
                payoff = F(payoff + ev)
                for a, cfv in actions:
                    regrets[a] = F(regrets.get(a, F(0.0)) + F(cfv - ev))
        return regrets, payoff

    def step(self):
        p = self.profile
        walker = p.t % 2
        nodes, frontiers = self.build(walker)
        for n in frontiers:
            n.payoffs = self.frontier_payoffs(n)
        self.counters["nodes"] += len(nodes)
        self.counters["frontiers"] += len(frontiers)
        self.counters["rollouts"] += len(frontiers) * 16 * self.rollouts
        partition = {}
        for n in nodes:
            if n.kids:
                partition.setdefault(n.info if n.info is not None else ("chance", n.index), []).append(n)
        if sum(1 for k in partition if k[0] != "chance") > MAX_INFOS:
            raise Malformed(NODES)
        updates = []
        for info, span in partition.items():  # ascending head-node order: dicts keep insertion order
            self.spans.append((p.t, walker, info, [n.index for n in span], self.turn(span[0])))
            if self.turn(span[0]) != walker:
                continue
            regret, payoff = self.dfs(span, walker)
            updates.append((info, regret, p.iterated(info), payoff))
        with np.errstate(all="ignore"):
            for info, regret, policy, payoff in updates:
                if info not in p.local and len(p.local) >= MAX_ROWS:
                    raise Malformed(ROWS)
                for a, delta in sorted(regret.items()):  # update_regret: SummedRegret::gain, floor -inf
                    total = p.cum(info, a, "regret")
                    p.mut(info, a)["regret"] = np.fmax(F(total + delta), F(-np.inf))
                for a, delta in enumerate(policy):  # update_weight: LinearWeight::learn
                    total = p.cum(info, a, "weight")
                    p.mut(info, a)["weight"] = np.fmax(F(total + F(delta * F(p.t))), EPS)
                for a in range(p.n(info)):  # update_payoff: Welford
                    n = p.cum(info, a, "visits")
                    e = p.mut(info, a)
                    e["payoff"] = F(e["payoff"] + F(F(payoff - e["payoff"]) / F(n + 1)))
                for a in range(p.n(info)):  # update_visits
                    p.mut(info, a)["visits"] += 1
        self.counters["infosets"] += len(updates)
        self.trees.append(nodes)
        p.t += 1

    def harvest(self):
        """-> dict: the Harvest at DepthInfo::Game(info of the entry state), the counters, the rows"""
        p = self.profile
        out = {"status": OK, "past": 0, "present": 0, "choices": 0, "n_actions": 0, "refined": np.zeros(A, F), "visits": np.zeros(A, np.uint32),
               "regret": F(0.0), "sum_regret": p.sum_regret(), "iterations": p.t, **self.counters}
        if inner_turn(self.game) >= 0:
            info = (GAME,) + FM.key_at(self.game, list(self.entry.prefix), inner_turn(self.game))
            n = p.n(info)
            out.update(past=info[1], present=info[2], choices=info[3], n_actions=n)
            out["refined"][:n] = p.iterated(info)
            out["visits"][:n] = [p.cum(info, a, "visits") for a in range(n)]
            out["regret"] = fold(np.fmax(p.cum(info, a, "regret"), F(0.0)) for a in range(n))
        rows = []
        for info in p.sorted_infos():
            enc = np.zeros(A, dtype=[("weight", "<f4"), ("regret", "<f4"), ("payoff", "<f4"), ("visits", "<u4")])
            for a, e in p.local[info].items():
                enc[a] = (e["weight"], e["regret"], e["payoff"], e["visits"])
            rows.append((info[0], p.n(info), info[1], info[2], info[3], enc))
        out["rows"], out["n_rows"] = rows, len(rows)
        return out


def failed(status):
    return {"status": status, "past": 0, "present": 0, "choices": 0, "n_actions": 0, "refined": np.zeros(A, F), "visits": np.zeros(A, np.uint32),
            "regret": F(0.0), "sum_regret": F(0.0), "iterations": 0, "nodes": 0, "infosets": 0, "frontiers": 0, "rollouts": 0, "rows": [],
            "n_rows": 0}


def solve(entry, origin, bp, index=0, iterations=1, keep=None, **kw):
    """one entry of a batch -> harvest dict; a malformed entry, or one that outgrows a cap, answers zeros and its status.
    keep: a list the Solve is appended to (the tests look at its trees)"""
    try:
        if origin is None:
            origin = street(FM.frontier_game(entry))
        if not -1 <= origin <= 3:
            raise Malformed(FM.SEAT)
        s = Solve(entry, origin, bp, index, **kw)
        if keep is not None:
            keep.append(s)
        for _ in range(iterations):
            s.step()
        return s.harvest()
    except Malformed as m:
        return failed(m.status)


# ---- a blueprint for the tests ----
ENC = np.dtype([("weight", "<f4"), ("regret", "<f4"), ("payoff", "<f4"), ("visits", "<u4")])
WEIGHTS = np.array([0.0, 1e-39, 1.0, 1e12], F)  # 1e-39 is subnormal: below RP_EPSILON
REGRETS = np.array([-3.0, 0.0, 2.5, 40.0], F)
PAYOFFS = np.array([-1.5, 0.0, 2.5, 7.25], F)
VISITS = np.array([0, 3, 11, 100], np.uint32)


class Blueprint:
    """the blueprint the model reads, decided key by key as the model asks (tests/test_gpu_nlhe_frontier.py's Rows with whole
    Encounters): about half of the keys get a row of corner values (garbage beyond the infoset's actions), one in eight of those with
    all-zero weights; the others — and every key asked for while `forbid` is set — have none"""

    def __init__(self, dense=False):
        self.loaded, self.never, self.forbid, self.dense = {}, set(), False, dense  # dense: every key asked for gets a row

    def enc(self, key):
        if self.forbid:
            self.never.add(key)
        if key in self.never:
            return None
        if key not in self.loaded:
            h = PM.key_hash(key[0] ^ 0x5EED, key[2], key[1])
            row = None
            if h % 2 == 0 or self.dense:
                row = np.zeros(A, ENC)
                for a in range(A):
                    x = (h >> (8 + 6 * a)) & 63
                    row[a] = (WEIGHTS[x & 3], REGRETS[(x >> 2) & 3], PAYOFFS[(x >> 4) & 3], VISITS[(x ^ (x >> 3)) & 3])
                if (h >> 4) % 8 == 0:
                    row["weight"] = 0.0
                n = PM.nch(key[2])
                row["weight"][n:], row["regret"][n:], row["payoff"][n:], row["visits"][n:] = 7.0, -9.0, 3.0, 5
            self.loaded[key] = row
        return self.loaded[key]

    def get(self, key):
        row = self.enc(key)
        return None if row is None else row["weight"]

    def table(self):
        keys = [k for k, r in self.loaded.items() if r is not None]
        enc = np.stack([self.loaded[k] for k in keys]) if keys else np.zeros((0, A), ENC)
        return (np.array([k[0] for k in keys], np.uint64), np.array([k[1] for k in keys], np.uint32),
                np.array([k[2] for k in keys], np.uint64), enc)

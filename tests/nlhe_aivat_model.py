"""The model the AIVAT tests compare against (helper, no tests): rp_nlhe_aivat (include/rp_mi355x.h) by the NAIVE algorithm of the
reference (arena/src/aivat.rs:63-229, correction.rs:4-22, replay.rs:90-168, repository.rs:397-442) over the CPU oracle's rules engine.

Two ora_games advance together: the walker, and a Witness that is a LIST OF ACTIONS replayed from its root every time something is
asked of it — head(), states(), history(), subgame(), aggression() are restated from kicker/src/recall.rs:43-112 as they are
written, each from scratch, so that the three aggression counts the kernel keeps incrementally (csrc/nlmc_aivat.hpp) are checked
against their definitions.  A chance node literally builds the deal list, the per-deal buckets, the DISTINCT buckets with their
baselines and the join, so that it checks the kernel's one-lane-per-deal shortcut.  Sums are numpy float32 left folds from 0.0.

A hand is any object with the attributes of robopoker_amd.nlhe.AivatHand.  rows.get((past, present, choices)) answers
(weights float32[9], payoffs float32[9]) or None: a dict will do."""
from __future__ import annotations

import ctypes as C

import numpy as np

import nlhe_policy_model as PM
import nlhe_range_model as RM
import oracle_nlhe as ON

F = np.float32
MAX_PLAYS, MAX_PATH = 48, 12
OK, EDGE, ILLEGAL, LENGTH, CARDS, DRAW, SEAT, LOOKUP = range(8)  # rp_recall_status
WITNESS = 11  # RP_AIVAT_WITNESS
KIND = {"fold": ON.FOLD, "call": ON.CALL, "check": ON.CHECK, "raise": ON.RAISE, "shove": ON.SHOVE}
FULL = (1 << 52) - 1
Malformed, popcount = RM.Malformed, RM.popcount


def _o():
    o = ON.lib()
    o.ora_nlhe_force_apply.restype = None
    o.ora_nlhe_force_apply.argtypes = [C.POINTER(ON.GameStruct), C.POINTER(ON.ActionStruct)]
    return o


def _copy(g):
    s = ON.GameStruct()
    C.memmove(C.byref(s), C.byref(g), C.sizeof(ON.GameStruct))
    return s


def _start(dealer, stacks, holes):
    g = ON.GameStruct()
    _o().ora_nlhe_from_start(C.byref(g), 2, dealer, (C.c_int16 * 2)(*stacks), (C.c_uint64 * 2)(*holes))
    return g


def _consume(g, a):
    """Game::consume: act without asking (kicker/src/game.rs:227-230)"""
    g = _copy(g)
    _o().ora_nlhe_force_apply(C.byref(g), C.byref(ON.ActionStruct(*a)))
    return g


def _allowed(g, a):
    return bool(_o().ora_nlhe_is_allowed(C.byref(g), C.byref(ON.ActionStruct(*a))))


def _turn(g):
    return _o().ora_nlhe_turn(C.byref(g))


def _street(g):
    return _o().ora_nlhe_street(C.byref(g))


def _edgify(g, a, depth):
    return _o().ora_nlhe_edgify(C.byref(g), C.byref(ON.ActionStruct(*a)), depth)


def _aggro_edge(e):
    return e == ON.E_SHOVE or e >= 6


def path_aggression(edges):
    """Path::aggression (kicker/src/path.rs:32-38) of a Path built from `edges`: Path keeps the FIRST 12"""
    n = 0
    for e in reversed(edges[:MAX_PATH]):
        if e == ON.E_DRAW:
            break
        n += _aggro_edge(e)
    return n


class Witness:
    """kicker/src/witness.rs as far as Aivat uses it: try_arrange(pov, arrangement, []) is stacks [STACK; 2] and dealer 0"""

    def __init__(self, hole, draws):
        self.hole, self.reveals, self.actions = hole, [d for d in draws if d], []

    def root(self):
        return _start(0, (ON.STACK, ON.STACK), (self.hole, self.hole))  # base(): every seat wiped to the pov's hole, then the blinds

    def states(self):
        out = [self.root()]
        for a in self.actions:
            out.append(_consume(out[-1], a))
        return out

    def head(self):
        return self.states()[-1]

    def seen_street(self):
        return len(self.reveals)

    def aggression(self):
        n = 0
        for a in reversed(self.actions):
            if a[0] == ON.DRAW:
                break
            n += a[0] in (ON.RAISE, ON.SHOVE)
        return n

    def history(self):
        past, out = [], []
        for g, a in zip(self.states(), self.actions):
            e = _edgify(g, a, path_aggression(past))
            past = (past + [e])[:MAX_PATH]
            out.append(e)
        return out

    def subgame(self):
        tail = []
        for e in reversed(self.history()):
            if e == ON.E_DRAW:
                break
            tail.append(e)
        return tail[::-1][:MAX_PATH]

    def info(self):
        """NlheInfo::from((recall, _)) (nlhe/src/info.rs:117-122): (past, choices) as the key's u64s"""
        sub = self.subgame()
        past, choices = C.c_uint64(), C.c_uint64()
        _o().ora_nlhe_info(C.byref(self.head()), ON.path_pack(sub), C.byref(past), C.byref(choices))
        assert past.value == ON.path_pack(sub)
        return past.value, choices.value

    def can_push(self, a):
        return _allowed(self.head(), a)

    def push(self, a):
        self.actions.append(a)
        while _street(self.head()) < self.seen_street() and _turn(self.head()) == ON.CHANCE:  # sprout
            self.actions.append(ON.Draw(self.reveals[_street(self.head())]))


def fold32(xs):
    s = F(0.0)
    for x in xs:
        s = F(s + F(x))
    return s


def strategy_ev(policy):
    total = fold32(w for w, _ in policy)
    if total <= 0:
        return F(0.0)
    return fold32(F(F(w / total) * v) for w, v in policy)


def observed_ev(policy, idx):
    return policy[idx][1] if idx is not None and idx < len(policy) else strategy_ev(policy)


def action_correction(policy, idx):
    with np.errstate(all="ignore"):
        return F(strategy_ev(policy) - observed_ev(policy, idx))


def chance_correction(avg, obs):
    with np.errstate(all="ignore"):
        return F(F(avg) - F(obs))


def validate(h):
    if len(h.plays) > MAX_PLAYS:
        raise Malformed(LENGTH)
    if h.seat > 1 or h.dealer > 1 or h.board_mode > 1 or (tuple(h.stacks) != (0, 0) and min(h.stacks) <= 0):
        raise Malformed(SEAT)
    gone = 0
    for hole in h.holes:
        if hole & ~FULL or popcount(hole) != 2 or hole & gone:
            raise Malformed(CARDS)
        gone |= hole
    draws = list(h.draws) + [0] * (3 - len(h.draws))
    for s, d in enumerate(draws):
        if d == 0:
            continue
        if d & ~FULL or popcount(d) != (3 if s == 0 else 1) or d & gone or (s > 0 and draws[s - 1] == 0):
            raise Malformed(CARDS)
        gone |= d
    plays = [(KIND.get(k, k), c) for k, c in h.plays]
    if any(k not in KIND.values() for k, _ in plays):
        raise Malformed(EDGE)
    return draws, [(k, 0 if k in (ON.FOLD, ON.CHECK) else c, 0) for k, c in plays]


def nearest_below(g, chips, depth):
    """the grid edge of (street, depth) with the most chips not above `chips` (what a floor would snap to), or None"""
    o = _o()
    best = None
    for e in ON.edge_raises(_street(g), depth):
        c = o.ora_edge_into_chips(e, g.pot)
        if c <= chips and (best is None or c > best[0]):
            best = (c, e)
    return best[1] if best else None


def action_node(recall, pocket, board, street, walker, action, rows, trace, node_street, bucket):
    key_pc = recall.info()
    key = (key_pc[0], bucket(street, pocket, board), key_pc[1])  # bucket None: eval_abstraction finds no row
    n = PM.nch(key[2])
    edge = _edgify(walker, action, recall.aggression())
    ev = dict(kind="action", key=key, street=node_street, found=False, zero=False, idx=None, edge=edge, value=None,
              below=nearest_below(walker, action[1], recall.aggression()) if action[0] == ON.RAISE else None)
    if trace is not None:
        trace.append(ev)
    row = rows.get(key) if n and key[1] is not None else None
    if row is None:
        return None
    ev["found"] = True
    policy = [(F(row[0][a]), F(row[1][a])) for a in range(n)]
    if fold32(w for w, _ in policy) <= 0:
        ev["zero"] = True
        return None
    slots = list(PM.edges(key[2])[:n])
    ev["idx"] = slots.index(edge) if edge in slots else None
    ev["value"] = action_correction(policy, ev["idx"])
    return ev["value"]


def chance_node(hero_recall, villain_recall, walker, holes, seat, observed, rows, trace, bucket):
    board = walker.board
    mask = holes[0] | holes[1] | board
    deals = [1 << c for c in range(52) if not mask >> c & 1]  # HandIterator::from((1, mask)): ascending
    sample = _consume(walker, ON.Draw(deals[0]))
    nxt = _turn(sample)
    ev = dict(kind="chance", dropped=0, null=0, value=None, sign=0, deals=0, obs_row=False, keys=[])
    if trace is not None:
        trace.append(ev)
    if nxt < 0:
        return None
    hero_next = nxt == seat
    recall, pocket = (hero_recall, holes[seat]) if hero_next else (villain_recall, holes[1 - seat])
    ev["sign"], ev["deals"] = (1 if hero_next else -1), len(deals)
    street = _street(walker) + 1
    past, choices = recall.info()
    n = PM.nch(choices)
    buckets = [bucket(street, pocket, board | d) for d in deals]  # deal_buckets; None: the isomorphism table has no row, the join drops the deal
    per_bucket = {}
    for b in dict.fromkeys(b for b in buckets if b is not None):  # SELECT DISTINCT abs ... JOIN blueprint ... GROUP BY abs
        row = rows.get((past, b, choices)) if n else None
        ev["keys"].append(((past, b, choices), row is not None))
        if row is None:
            continue
        with np.errstate(all="ignore"):
            sw = fold32(row[0][:n])
            swv = fold32(F(F(row[0][a]) * F(row[1][a])) for a in range(n))
            per_bucket[b] = None if sw == 0 else F(swv / sw)
    joined = [per_bucket[b] for b in buckets if b in per_bucket]
    ev["dropped"], ev["null"] = len(buckets) - len(joined), sum(x is None for x in joined)
    ob = bucket(street, pocket, board | observed)
    ev["obs_row"] = ob in per_bucket
    obs = per_bucket.get(ob)
    values = [x for x in joined if x is not None]
    if not values or obs is None:
        return None
    with np.errstate(all="ignore"):
        avg = F(np.float64(fold32(values)) / np.float64(len(joined)))
        delta = chance_correction(avg, obs)
        ev["value"] = delta if hero_next else F(-delta)
    return ev["value"]


def corrections(h, rows, trace=None, bucket=RM._bucket):
    """-> (status, hero, villain, chance, total, n_action, n_chance); a refused hand: its status and zeros.  bucket(street, pocket,
    board) -> the abstraction, or None where the encoder's tables do not hold the observation (default: the hash encoder)"""
    zero = (F(0.0),) * 4 + (0, 0)
    try:
        draws, plays = validate(h)
        stacks = tuple(h.stacks) if tuple(h.stacks) != (0, 0) else (ON.STACK, ON.STACK)
        walker = _start(h.dealer, stacks, h.holes)
        seat, other = h.seat, 1 - h.seat
        hero_recall, villain_recall = Witness(h.holes[seat], draws), Witness(h.holes[other], draws)
        all_board = draws[0] | draws[1] | draws[2]
        hero = villain = chance = F(0.0)
        n_action = n_chance = 0
        for a in plays:
            if _turn(walker) == ON.TERMINAL:
                break
            while _turn(walker) == ON.CHANCE:
                s = _street(walker)
                if draws[s] == 0:
                    raise Malformed(DRAW)
                if s != 0:
                    d = chance_node(hero_recall, villain_recall, walker, h.holes, seat, draws[s], rows, trace, bucket)
                    if d is not None:
                        with np.errstate(all="ignore"):
                            chance = F(chance + d)
                        n_chance += 1
                walker = _consume(walker, ON.Draw(draws[s]))
            for who, recall in ((seat, hero_recall), (other, villain_recall)):
                if _turn(walker) == who:
                    at_node = h.board_mode == 1
                    d = action_node(recall, h.holes[who], walker.board if at_node else all_board,
                                    _street(walker) if at_node else recall.seen_street(), walker, a, rows, trace, _street(walker), bucket)
                    if d is not None:
                        with np.errstate(all="ignore"):
                            if who == seat:
                                hero = F(hero + d)
                            else:
                                villain = F(villain - d)
                        n_action += 1
            if not hero_recall.can_push(a):
                raise Malformed(WITNESS if _allowed(walker, a) else ILLEGAL)
            assert villain_recall.can_push(a)
            hero_recall.push(a)
            villain_recall.push(a)
            if not _allowed(walker, a):
                raise Malformed(ILLEGAL)
            walker = _consume(walker, a)
    except Malformed as m:
        return (m.status,) + zero
    with np.errstate(all="ignore"):
        total = F(F(hero + villain) + chance)
    return OK, hero, villain, chance, total, n_action, n_chance


class Recorder:
    """an empty blueprint that remembers what it was asked"""

    def __init__(self):
        self.asked = {}  # a dict for its order

    def get(self, key):
        self.asked.setdefault(key, None)
        return None


def summarize(adjusted, raw_stddev):
    """Aivat::summarize (aivat.rs:45-61) with ratio / erf of pokerkit/src/metrics.rs:102-119; exp is glibc's expf"""
    expf = C.CDLL("libm.so.6").expf  # glibc's, which include/rp_libm_glibc.h restates bit for bit
    expf.restype, expf.argtypes = C.c_float, [C.c_float]
    ratio = lambda a, b: F(a / b) if b > 0 else F(0.0)  # noqa: E731
    x = [F(v) for v in adjusted]
    with np.errstate(all="ignore"):
        n = F(len(x))
        won = fold32(x)
        mean = ratio(won, n)
        variance = ratio(fold32(F(F(v - mean) * F(v - mean)) for v in x), n)
        stderr = ratio(np.sqrt(variance), np.sqrt(n))
        raw = F(F(raw_stddev) * F(raw_stddev))
        adj = F(F(stderr * stderr) * n)

        def erf(z):
            a, b, c, d, e, f, g = (F(v) for v in (0.2316419, 0.3989423, 0.3193815, -0.3565638, 1.781478, -1.821256, 1.330274))
            t = F(F(1.0) / F(F(1.0) + F(a * abs(z))))
            arg = F(F(F(-z) * z) / F(2.0))
            dd = F(b * F(expf(float(arg))))
            p = F(F(dd * t) * F(c + F(t * F(d + F(t * F(e + F(t * F(f + F(t * g)))))))))
            return F(F(1.0) - p) if z > 0 else p

        reduction = F(raw / adj) if adj > 0 else F(1.0)
        pvalue = F(F(2.0) * erf(F(F(-abs(mean)) / stderr))) if stderr > 0 else F(1.0)
    return dict(won=won, mean=mean, stderr=stderr, reduction=reduction, pvalue=pvalue)

"""The model the match tests compare against (helper, no tests): rp_nlhe_match (include/rp_mi355x.h) by the NAIVE algorithm of the
reference's table (parlor/src/engine.rs:48-68, 268-320; players/{agent,brain,dirac,fish}.rs) over the CPU oracle's rules engine.

Every decision builds the engine's Witness anew — the real buy-ins and dealer, the actor's hole, the streets dealt so far, the choice
actions pushed one by one — as a LIST OF ACTIONS replayed from its root for every subgame() / aggression() (the Witness of
nlhe_aivat_model.py on another root), so that the counters the kernel keeps incrementally beside its one game (csrc/nlmc_match.hpp)
are checked against their definitions.  The policy is a literal dict sorted by an Edge key built from the reference's DECLARATION
order (kicker/src/edge.rs:18-27, odds.rs:10-11), which is what #[derive(Ord)] compares and a BTreeMap iterates in; the kernel's rank
table is not used.  Sums are numpy float32 left folds; the random numbers are the counter contract of nlhe_rollout_model.py.

rows.get((past, present, choices)) answers weights float32[9] or None: a dict will do."""
from __future__ import annotations

import ctypes as C

import numpy as np

import nlhe_aivat_model as AM
import nlhe_policy_model as PM
import nlhe_range_model as RM
import nlhe_rollout_model as RO
import oracle_nlhe as ON

F = np.float32
OK, EDGE, ILLEGAL, LENGTH, CARDS, DRAW, SEAT, LOOKUP = range(8)  # rp_recall_status
BLUEPRINT, DIRAC, FISH = range(3)  # rp_agent_kind
AGENT = {"blueprint": BLUEPRINT, "dirac": DIRAC, "fish": FISH}
MAX_PLAYS, MAX_STEPS = 48, RO.MAX_STEPS
VARIANTS = ["Draw", "Fold", "Check", "Call", "Open", "Raise", "Shove"]  # enum Edge, as declared


def edge_key(code: int):
    """what #[derive(Ord)] compares: the variant's place in the declaration, then its payload (Open: chips; Raise: Odds(n, d))"""
    if code >= 10:
        return (VARIANTS.index("Raise"),) + ON.RAISES[code - 10]
    if code >= 6:
        return (VARIANTS.index("Open"), ON.OPENS[code - 6])
    return (VARIANTS.index({ON.E_DRAW: "Draw", ON.E_FOLD: "Fold", ON.E_CHECK: "Check", ON.E_CALL: "Call", ON.E_SHOVE: "Shove"}[code]),)


class Args:
    """rp_nlhe_match_args"""

    def __init__(self, seed=0, first_id=0, stacks=(0, 0), agents=("blueprint", "blueprint"), dealer=2, hero=0, mirror=False, snap=False,
                 board_mode=1):
        self.seed, self.first_id, self.stacks, self.dealer, self.hero = seed, first_id, tuple(stacks), dealer, hero
        self.agents = tuple(AGENT[k] if isinstance(k, str) else k for k in agents)
        self.mirror, self.snap, self.board_mode = bool(mirror), bool(snap), board_mode

    def kwargs(self):
        return dict(seed=self.seed, first_id=self.first_id, stacks=self.stacks, agents=self.agents, dealer=self.dealer, hero=self.hero,
                    mirror=self.mirror, snap=self.snap, board_mode=self.board_mode)


class TableWitness(AM.Witness):
    """Witness::initial_with(pov, arrangement, buyins, dealer): the Witness of the AIVAT model on the table's own root"""

    def __init__(self, hole, reveals, stacks, dealer):
        super().__init__(hole, reveals)
        self.stacks, self.dealer = stacks, dealer

    def root(self):
        return AM._start(self.dealer, self.stacks, (self.hole, self.hole))


def deal(seed: int, deal_id: int):
    """-> (hole of seat 0, hole of seat 1, [flop, turn, river]): nine cards, each the pick-th lowest of the deck, which loses it"""
    deck = list(range(52))
    cards = [1 << deck.pop(RO.pick_uniform(RO.node_hash(seed, 0, deal_id, c), len(deck))) for c in range(9)]
    return cards[0] | cards[1], cards[2] | cards[3], [cards[4] | cards[5] | cards[6], cards[7], cards[8]]


def sample(policy: dict, u) -> int:
    """WeightedIndex over the BTreeMap's values in key order, as the header fixes its arithmetic -> the edge"""
    items = sorted(policy.items())
    with np.errstate(all="ignore"):
        total = F(0.0)
        for _, (_, p) in items:
            total = F(total + F(p))
        threshold = F(F(u) * total)
        acc = F(0.0)
        for _, (edge, p) in items:
            acc = F(acc + F(p))
            if threshold < acc:
                return edge
    return items[-1][1][0]


def argmax(policy: dict) -> int:
    """nlhe::argmax: Iterator::max_by with ties Equal keeps the LAST maximal element in key order -> the edge"""
    best = None
    for _, (edge, p) in sorted(policy.items()):
        if best is None or not best[1] > p:
            best = (edge, p)
    return best[0]


def fish(game, draw: int):
    """Fish::decide: legal() without the shove, one of them uniformly"""
    g = ON.Game(game, None)
    options = [a for a in g.legal() if a[0] != ON.SHOVE]
    if not options:
        raise RM.Malformed(ILLEGAL)
    return options[RO.pick_uniform(draw, len(options))]


def play(hand_id: int, args: Args, rows, bucket=RM._bucket, trace=None):
    """one hand -> dict(status, holes, draws, stacks, dealer, seat, board_mode, plays [(kind, chips)], n_plays, won, rejected);
    rows: the blueprints of seat 0 and seat 1; trace collects one dict per decision"""
    o = AM._o()
    hand_id &= RO.M64
    zero = dict(holes=(0, 0), draws=(0, 0, 0), stacks=(0, 0), dealer=0, seat=0, board_mode=0, plays=[], n_plays=0, won=0, rejected=0)
    hole0, hole1, streets = deal(args.seed, hand_id >> 1 if args.mirror else hand_id)
    if args.mirror and hand_id & 1:
        hole0, hole1 = hole1, hole0
    holes = (hole0, hole1)
    dealer = hand_id & 1 if args.dealer == 2 else args.dealer
    stacks = args.stacks if args.stacks != (0, 0) else (ON.STACK, ON.STACK)
    live = AM._start(dealer, stacks, holes)
    plays, dealt, rejected, decision = [], [], 0, 0
    try:
        for _ in range(MAX_STEPS):
            turn = AM._turn(live)
            if turn == ON.TERMINAL:
                won = ON.Game(live, None).settlements()[args.hero][1]
                status = LENGTH if len(plays) > MAX_PLAYS else OK
                kept = plays[:MAX_PLAYS]
                return dict(status=status, holes=holes, draws=tuple(dealt + [0] * (3 - len(dealt))), stacks=args.stacks, dealer=dealer,
                            seat=args.hero, board_mode=args.board_mode,
                            plays=[(k, 0 if k in (ON.FOLD, ON.CHECK) else c) for k, c, _ in kept], n_plays=len(kept), won=won, rejected=rejected)
            if turn == ON.CHANCE:
                dealt.append(streets[AM._street(live)])
                live = AM._consume(live, ON.Draw(dealt[-1]))
                continue
            draw = RO.node_hash(args.seed, 1, hand_id, decision)
            decision += 1
            ev = dict(hand=hand_id, seat=turn, agent=args.agents[turn], street=AM._street(live), rejected=False, n_before=len(plays) + len(dealt))
            if trace is not None:
                trace.append(ev)
            if args.agents[turn] == FISH:
                action = fish(live, draw)
            else:
                recall = TableWitness(holes[turn], dealt, stacks, dealer)
                for a in plays:
                    recall.push(a)
                past, choices = recall.info()
                ev["street_edges"] = len(recall.subgame())
                n = PM.nch(choices)
                if n == 0:
                    raise RM.Malformed(ILLEGAL)
                present = bucket(AM._street(live), holes[turn], live.board)
                if present is None:
                    raise RM.Malformed(LOOKUP)
                key = (past, present, choices)
                w = rows[turn].get(key)
                dist = PM.distribution("averaged", np.zeros(PM.A, F) if w is None else w, n)[:n]
                slots = [int(e) for e in PM.edges(choices)[:n]]
                policy = {edge_key(e): (e, F(p)) for e, p in zip(slots, dist)}  # the BTreeMap<Edge, Probability>
                edge = argmax(policy) if args.agents[turn] == DIRAC else sample(policy, RO.u01(draw))
                ev.update(key=key, found=w is not None, slots=slots, ordered=[e for _, (e, _) in sorted(policy.items())], edge=edge,
                          by_slot_order=sample({(i,): (e, F(p)) for i, (e, p) in enumerate(zip(slots, dist))}, RO.u01(draw)))
                r = o.ora_nlhe_actionize(C.byref(live), edge, 0)
                action = (r.kind, 0 if r.kind in (ON.FOLD, ON.CHECK) else r.chips, 0)
            ev["asked"] = action
            if args.snap:
                action = ON.Game(live, None).snap(action)
                if not AM._allowed(live, action):
                    raise RM.Malformed(ILLEGAL)
            elif not AM._allowed(live, action):  # rejected: the seat times out into passive()
                action = ON.Check if ON.Game(live, None).may_check else ON.Fold
                rejected = min(rejected + 1, 255)
                ev["rejected"] = True
            ev["action"] = action
            plays.append(action)
            live = AM._consume(live, action)
        raise RM.Malformed(ILLEGAL)
    except RM.Malformed as m:
        return dict(zero, status=m.status)


def match(n: int, args: Args, rows, bucket=RM._bucket, trace=None):
    """the batch: a list of play()'s dicts for hand ids first_id .. first_id + n - 1"""
    return [play(args.first_id + i, args, rows, bucket, trace) for i in range(n)]


def summarize(won):
    """spar/src/benchmark.rs:122-147 on float64"""
    x = [np.float64(int(w)) / np.float64(ON.B_BLIND) for w in won]
    n = len(x)
    out = dict(hands=n, total_bb=np.float64(0.0), bb_per_100=np.float64(0.0), stddev=np.float64(0.0), confidence=np.float64(0.0))
    if n == 0:
        return out
    total = np.float64(0.0)
    for v in x:
        total = total + v
    out["total_bb"], out["bb_per_100"] = total, total / np.float64(n) * np.float64(100.0)
    if n >= 2:
        mean, squares = total / np.float64(n), np.float64(0.0)
        for v in x:
            squares = squares + (v - mean) * (v - mean)
        out["stddev"] = np.sqrt(squares / np.float64(n - 1))
    out["confidence"] = np.float64(1.96) * out["stddev"] / np.sqrt(np.float64(n)) * np.float64(100.0)
    return out

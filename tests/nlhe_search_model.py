"""The model the search-match tests compare against (helper, no tests): rp_nlhe_search_match (include/rp_mi355x.h) by the NAIVE
composition the header names — the table of nlhe_match_model.py, at whose postflop decisions a search seat asks
nlhe_world_model.belief and nlhe_subgame_model.solve for the recall it has witnessed and plays Solved::blend
(parlor/src/players/solved.rs:133-152) of the harvest and its blueprint, restated literally over np.float32 scalars.

The hand is nlhe_match_model.play's loop with that one hook; its pieces (the deal, the witness, the BTreeMap policy, sample, argmax,
fish) are that module's, not copies.  The recall is built from the Witness's own history() — the list of actions replayed from the
root — so that the history the kernel keeps edge by edge beside its game (csrc/nlmc_search.hpp) is checked against its definition.

rows: the blueprints of seat 0 and seat 1, each with get(key) -> weights float32[9] or None and enc(key) -> the whole Encounter row
or None (what the solver warm-starts from)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import nlhe_aivat_model as AM
import nlhe_match_model as MM
import nlhe_policy_model as PM
import nlhe_range_model as RM
import nlhe_rollout_model as RO
import nlhe_subgame_model as SM
import nlhe_world_model as WM
import oracle_nlhe as ON
from robopoker_amd.nlhe import Frontier, Recall

F = np.float32
EPS = PM.EPSILON
NONE, WORLD = 0, 1  # rp_search_kind
SEARCH = {"none": NONE, "world": WORLD}
SOLVED, BELIEF, SOLVE, KEY, LENGTH, CAP = range(6)  # rp_search_fallback
MAX_SOLVES, MAX_HISTORY, MAX_PREFIX = 48, 48, 12


class SearchArgs:
    """rp_nlhe_search_args without its match"""

    def __init__(self, search=("none", "none"), origin_mode=0, iterations=1, rollouts=16, bias=5.0, prior=float(1 << 14), visit_threshold=1 << 18,
                 steps_cap=0, search_seed=0):
        self.search = tuple(SEARCH[k] if isinstance(k, str) else k for k in search)
        self.origin_mode, self.iterations, self.rollouts, self.bias, self.prior = origin_mode, iterations, rollouts, bias, prior
        self.visit_threshold, self.steps_cap, self.search_seed = visit_threshold, steps_cap, search_seed

    def kwargs(self):
        return dict(search=self.search, origin_mode=self.origin_mode, iterations=self.iterations, rollouts=self.rollouts, bias=self.bias,
                    prior=self.prior, visit_threshold=self.visit_threshold, steps_cap=self.steps_cap, search_seed=self.search_seed)


def blend(refined, visits, bp, slots, threshold):
    """Solved::blend -> p float32[n] by slot; the total folds over the BTreeMap's key order"""
    n = len(slots)
    with np.errstate(all="ignore"):
        raw = []
        for a in range(n):
            v = F(int(visits[a]))
            w = F(v / F(v + F(threshold)))
            raw.append(F(F(w * F(refined[a])) + F(F(F(1.0) - w) * F(bp[a]))))
        total = F(0.0)
        for a in sorted(range(n), key=lambda a: MM.edge_key(slots[a])):
            total = F(total + raw[a])
        total = max(total, F(EPS))
        return [F(r / total) for r in raw]


def search_decision(sargs, hand_id, decision, turn, recall_witness, stacks, dealer, dealt, hole, rows, bp_epoch, key, slots, bp):
    """one postflop decision of a search seat, asked for its solve -> the step dict (p: what the seat plays from)"""
    edges = recall_witness.history()
    solve_id = (hand_id * 256 + (decision & 255)) & RO.M64
    recall = Recall(turn, hole, dealt, edges, stacks, dealer)
    holes = [0, 0]
    holes[turn] = hole
    entry = Frontier(holes, turn, dealt, edges, recall_witness.subgame()[:MAX_PREFIX], stacks, dealer)
    bel = WM.belief(recall, rows)
    street = len(dealt)
    origin = street - 1 if sargs.origin_mode else None
    res = SM.solve(entry, bel["hole_world"], bel["weights"], origin, rows, 0, sargs.iterations, bp_epoch=bp_epoch, rollouts=sargs.rollouts,
                   bias=sargs.bias, prior=sargs.prior, seed=sargs.search_seed, first_id=solve_id)
    if bel["status"] != RM.OK:
        code = BELIEF
    elif res["status"] != RM.OK:
        code = SOLVE
    elif (res["past"], res["present"], res["choices"]) != key:
        code = KEY
    else:
        code = SOLVED
    p = blend(res["refined"], res["visits"], bp, slots, sargs.visit_threshold) if code == SOLVED else list(bp)
    return dict(solve_id=solve_id, recall=recall, result=res, belief_status=bel["status"], bp=list(bp), p=p, seat=turn, decision=decision,
                fallback=code, entry=entry, belief=bel)


def play(hand_id: int, args: MM.Args, sargs: SearchArgs, rows, bp_epoch=0, bucket=RM._bucket):
    """one hand -> nlhe_match_model.play's dict plus searched, unsolved and steps (every search decision, uncapped)"""
    o = AM._o()
    hand_id &= RO.M64
    zero = dict(holes=(0, 0), draws=(0, 0, 0), stacks=(0, 0), dealer=0, seat=0, board_mode=0, plays=[], n_plays=0, won=0, rejected=0, searched=0,
                unsolved=0, steps=[])
    hole0, hole1, streets = MM.deal(args.seed, hand_id >> 1 if args.mirror else hand_id)
    if args.mirror and hand_id & 1:
        hole0, hole1 = hole1, hole0
    holes = (hole0, hole1)
    dealer = hand_id & 1 if args.dealer == 2 else args.dealer
    stacks = args.stacks if args.stacks != (0, 0) else (ON.STACK, ON.STACK)
    live = AM._start(dealer, stacks, holes)
    plays, dealt, rejected, decision, steps, solves, searched = [], [], 0, 0, [], 0, 0
    try:
        for _ in range(MM.MAX_STEPS):
            turn = AM._turn(live)
            if turn == ON.TERMINAL:
                won = ON.Game(live, None).settlements()[args.hero][1]
                kept = plays[:MM.MAX_PLAYS]
                return dict(status=MM.LENGTH if len(plays) > MM.MAX_PLAYS else MM.OK, holes=holes, draws=tuple(dealt + [0] * (3 - len(dealt))),
                            stacks=args.stacks, dealer=dealer, seat=args.hero, board_mode=args.board_mode,
                            plays=[(k, 0 if k in (ON.FOLD, ON.CHECK) else c) for k, c, _ in kept], n_plays=len(kept), won=won, rejected=rejected,
                            searched=min(searched, 255), unsolved=min(sum(s["fallback"] != SOLVED for s in steps), 255), steps=steps)
            if turn == ON.CHANCE:
                dealt.append(streets[AM._street(live)])
                live = AM._consume(live, ON.Draw(dealt[-1]))
                continue
            draw = RO.node_hash(args.seed, 1, hand_id, decision)
            if args.agents[turn] == MM.FISH:
                action = MM.fish(live, draw)
            else:
                recall = MM.TableWitness(holes[turn], dealt, stacks, dealer)
                for a in plays:
                    recall.push(a)
                past, choices = recall.info()
                n = PM.nch(choices)
                if n == 0:
                    raise RM.Malformed(MM.ILLEGAL)
                street = AM._street(live)
                present = bucket(street, holes[turn], live.board)
                if present is None:
                    raise RM.Malformed(MM.LOOKUP)
                key = (past, present, choices)
                w = rows[turn].get(key)
                dist = [F(x) for x in PM.distribution("averaged", np.zeros(PM.A, F) if w is None else w, n)[:n]]
                slots = [int(e) for e in PM.edges(choices)[:n]]
                step = None
                if sargs.search[turn] != NONE and street > 0:
                    searched += 1
                    n_edges = len(recall.history())
                    code = LENGTH if n_edges > MAX_HISTORY else CAP if solves >= MAX_SOLVES else SOLVED
                    if code != SOLVED:  # no solve is asked for
                        step = dict(solve_id=(hand_id * 256 + (decision & 255)) & RO.M64, recall=None, result=None, belief_status=0, bp=dist,
                                    p=dist, seat=turn, decision=decision, fallback=code)
                    else:
                        solves += 1
                        step = search_decision(sargs, hand_id, decision, turn, recall, args.stacks, dealer, list(dealt), holes[turn], rows[turn],
                                               bp_epoch, key, slots, dist)
                    steps.append(step)
                    dist = step["p"]
                policy = {MM.edge_key(e): (e, F(p)) for e, p in zip(slots, dist)}  # the BTreeMap<Edge, Probability>
                edge = MM.argmax(policy) if args.agents[turn] == MM.DIRAC else MM.sample(policy, RO.u01(draw))
                if step is not None:
                    step["edge"] = edge
                    step["bp_edge"] = (MM.argmax if args.agents[turn] == MM.DIRAC else lambda q: MM.sample(q, RO.u01(draw)))(
                        {MM.edge_key(e): (e, F(p)) for e, p in zip(slots, step["bp"])})
                    step["dirac_tie"] = args.agents[turn] == MM.DIRAC and sum(F(p) == max(F(x) for x in dist) for p in dist) > 1
                r = o.ora_nlhe_actionize(C.byref(live), edge, 0)
                action = (r.kind, 0 if r.kind in (ON.FOLD, ON.CHECK) else r.chips, 0)
            decision += 1
            if args.snap:
                action = ON.Game(live, None).snap(action)
                if not AM._allowed(live, action):
                    raise RM.Malformed(MM.ILLEGAL)
            elif not AM._allowed(live, action):  # rejected: the seat times out into passive()
                action = ON.Check if ON.Game(live, None).may_check else ON.Fold
                rejected = min(rejected + 1, 255)
            plays.append(action)
            live = AM._consume(live, action)
        raise RM.Malformed(MM.ILLEGAL)
    except RM.Malformed as m:
        return dict(zero, status=m.status)


def match(n: int, args: MM.Args, sargs: SearchArgs, rows, bp_epoch=0):
    return [play(args.first_id + i, args, sargs, rows, bp_epoch) for i in range(n)]

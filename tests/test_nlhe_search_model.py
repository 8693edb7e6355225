"""Pins the model of the search match (tests/nlhe_search_model.py) on the CPU, and asserts that the batches of
tests/nlhe_search_cases.py hold every case the kernels have to get right — what their seeds and first ids were searched for."""
import numpy as np

import nlhe_match_model as MM
import nlhe_search_cases as SC
import nlhe_search_model as XM
import nlhe_search_replay as RP
from robopoker_amd import _lib

F = np.float32


def test_the_symbol_the_model_stands_for_exists():
    assert hasattr(_lib.load(), "rp_nlhe_search_match")


def test_blend_is_solved_blend():
    slots = [MM.ON.E_CALL, MM.ON.E_FOLD, 12]  # slot order; Edge order is Fold < Call < Raise
    refined, visits, bp = [F(0.5), F(0.25), F(0.25)], [6, 0, 2], [F(0.2), F(0.3), F(0.5)]
    p = XM.blend(refined, visits, bp, slots, 2)
    w = [F(F(6) / F(8)), F(0), F(F(2) / F(4))]
    raw = [F(F(w[a] * refined[a]) + F(F(F(1) - w[a]) * bp[a])) for a in range(3)]
    total = F(F(F(0) + raw[1]) + raw[0]) + raw[2]
    assert [x.view(np.uint32) for x in p] == [F(r / F(total)).view(np.uint32) for r in raw]
    assert raw[1] == bp[1]  # no visit: the blueprint's probability
    zero = XM.blend([F(0)] * 2, [4, 4], [F(0)] * 2, slots[:2], 1)
    assert zero == [F(0), F(0)]  # the total is floored at EPSILON, not divided by zero
    # a threshold far above the visits leaves the blueprint
    far = XM.blend(refined, visits, bp, slots, 1 << 30)
    assert max(abs(float(a) - float(b)) for a, b in zip(far, bp)) < 1e-6


def test_without_a_search_seat_the_model_is_the_match_model():
    _, n, args, _, _ = SC.config("world blueprint")
    rows = SC.model().rows
    got = XM.match(n, args, XM.SearchArgs(), rows)
    want = MM.match(n, args, rows)
    for g, w in zip(got, want):
        assert {k: g[k] for k in w} == w and g["searched"] == g["unsolved"] == 0 and g["steps"] == []


def test_every_case_occurs():
    m = SC.model()
    steps = {name: m.all_steps(name) for name in SC.NAMES}
    every = [s for name in SC.NAMES for s in steps[name]]
    for name in SC.NAMES:
        n, hands = SC.config(name)[1], m.want[name]
        # every hand has outputs: on the hash encoder snap refuses nothing and no bucket is missing.  A hand refused after it has traced
        # a step needs lookup-table encoders: test_gpu_nlhe_search_match.py plays such hands against this model with the tables' buckets
        assert n == len(hands) <= 9 and all(w["status"] == MM.OK for w in hands), name
        solved = sum(s["fallback"] == XM.SOLVED for s in steps[name])
        assert steps[name] and 2 * solved >= len(steps[name]), (name, solved, len(steps[name]))  # the comparison is of solves, not of fallbacks
        assert max(len(w["steps"]) for w in hands) <= SC.STEPS_CAP, name  # every search decision is traced
        assert [w["searched"] for w in hands] == [len(w["steps"]) for w in hands]
        assert [w["unsolved"] for w in hands] == [sum(s["fallback"] != XM.SOLVED for s in w["steps"]) for w in hands]
    # a solved decision on each postflop street
    assert {len(s["recall"].draws) for s in every if s["fallback"] == XM.SOLVED} == {1, 2, 3}
    # The fallbacks the batches can reach.
    # SOLVE (a solve refused after a belief that was not) is in none of these batches, which are played on the hash encoder: it is
    # pinned on lookup-table encoders, against the replay model, by tests/test_gpu_nlhe_search_chunks.py
    # (test_a_solve_refused_after_a_belief_that_was_not: RP_RECALL_LOOKUP from a frontier's rollout, origin_mode 1).  On the hash encoder
    # no route was found.  Searched with the full model, both seats searching, 2 iterations, per solve (the counters add up over the
    # two trees, the caps are per tree):
    #   origin_mode 0 — 1 140 hands at stacks (0, 0) and 60 to 16 384: every solve RP_RECALL_OK; at most 104 nodes (RP_DEPTH_NODES: 384
    #     a tree), 19 infosets (96 a tree), 19 rows (RP_DEPTH_ROWS: 2 048 a solve).
    #   origin_mode 1 — 2 450 hands at (0, 0), 60 and 100: every solve RP_RECALL_OK; at most 205 nodes, 26 infosets, 26 rows and 22
    #     frontiers (RP_DEPTH_FRONTIERS: 32 a tree; 22 is the largest seen in the 264 solves that were counted).
    #   RP_DEPTH_ROWS by iterations — the first solve of 5 hands at 256 iterations: 419 to 708 rows of 2 048, in 2.2 to 3.9 s of
    #     model time each; the rows flatten, and the 5 s a config may cost is used up long before the cap.
    #   The raises a street admits bound the sampled tree well below every cap.
    # At stacks 24 000 and 32 767 the MODEL refuses solves (RP_RECALL_ILLEGAL) that the library plays: in the oracle's int16 chips a
    # raise over a shove wraps to a negative stack and the next node offers no edge.  The header states it (PINNED WHILE THE POT FITS
    # AN int16); those hands pin nothing and are in no batch.
    # LENGTH and CAP need 49 edges of history or 49 solves in one hand and are in none.  Searched with nlhe_match_model.play, no
    # solves, seed 7, stacks (32 767, 32 767), (32 767, 3 000) and (0, 0), dealer alternating: 100 000 ids for each of blueprint v
    # blueprint (snap off and on) and blueprint v dirac — 900 000 hands — met at most 21 edges at a postflop decision of a seat that
    # could search and at most 14 such decisions in a hand; 13 000 hands with a fish on one seat (blueprint or dirac on the other,
    # snap off and on) at most 18 and 7.  Pot-fraction raises grow the pot by a quarter at least, and a street admits few of them
    # (the largest sampled tree above): between two table agents the history is bounded far below 49.  A fish raises the minimum,
    # which grows the pot linearly — hands of 32 767 decisions and more were met at those stacks — so no bound is claimed against a
    # fish; none of those hands had a search seat's postflop decision past 18 edges.
    assert {s["fallback"] for s in every} == {XM.SOLVED, XM.BELIEF, XM.KEY}
    # the trace cap: hands of "both" and "deep" have three search decisions or more, so that a steps_cap of 1 and of one below the most
    # end the trace before the hand (tests/test_gpu_nlhe_search_chunks.py)
    assert all(max(len(w["steps"]) for w in m.want[name]) >= 3 for name in ("both", "deep"))
    fish = SC.config("world fish")[2]
    assert fish.agents[1] == MM.FISH and not fish.snap and any(s["fallback"] == XM.KEY for s in steps["world fish"])
    assert any(s["fallback"] == XM.BELIEF and s["belief_status"] != MM.OK for s in steps["world fish"])
    for s in every:  # a fallback plays the blueprint's policy
        assert (s["fallback"] == XM.SOLVED) or [F(x).view(np.uint32) for x in s["p"]] == [F(x).view(np.uint32) for x in s["bp"]]
    # Dirac's tie on a search decision; both Dirac and the sampling agent search somewhere
    assert any(s["dirac_tie"] for s in steps["fish dirac world"]) and SC.config("fish dirac world")[2].agents[1] == MM.DIRAC
    # a hand with both seats searching, on two tables and on one; the second table matters
    for name in ("both", "both one table"):
        assert any(len({s["seat"] for s in w["steps"]}) == 2 for w in m.want[name]), name
    differ = [a["plays"] != b["plays"] for a, b in zip(m.want["both"], m.want["both one table"])]
    assert 0 < sum(differ) < len(differ)
    # the solved play differs from the blueprint's for the same draw, and the blend moved the policy
    assert sum(s["edge"] != s["bp_edge"] for s in every if s["fallback"] == XM.SOLVED) >= 5
    assert all(any(F(a) != F(b) for a, b in zip(s["p"], s["bp"])) for s in every if s["fallback"] == XM.SOLVED and s["result"]["visits"].any())
    # origin_mode 1 plays rollouts where a street lies beyond the entry's; the reference's mode none
    assert any(s["result"]["rollouts"] > 0 for s in steps["origin"]) and not any(s["result"]["rollouts"] for s in steps["both"])
    # solve ids are the hand's and the decision's, never the batch's
    for name in SC.NAMES:
        first = SC.config(name)[2].first_id
        for i, w in enumerate(m.want[name]):
            assert all(s["solve_id"] == (first + i) * 256 + s["decision"] for s in w["steps"])
    assert len({s["solve_id"] for s in steps["both"]}) == len(steps["both"])
    assert (1 << m.cap_log2) >= 2 * max(t[0].size for t in m.tables)


def test_the_big_batch_fills_the_scan_in_its_first_round():
    """what tests/test_gpu_nlhe_search_chunks.py's 1 089 hands are for, as far as it can be said without a solve: the first round of a
    chunk asks for the first search decision of every hand that has one, and a hand gets there on its blueprint alone"""
    big = RP.big_batch()
    seat0, seat1 = big["first"]
    assert seat0 > 256 and seat1 > 256  # every thread of the 256-thread scan holds a request; seat 1's list starts past seat 0's
    assert seat0 + seat1 <= RP.CHUNK and RP.BIG_N == RP.CHUNK + 64 + 1 and big["args"].first_id == SC.config("both")[2].first_id
    assert big["sargs"].steps_cap == RP.BIG_CAP < 3 and tuple(big["sargs"].search) == (XM.WORLD, XM.WORLD)
    # the blueprints are nlhe_search_cases' with passive preflop rows added, none taken away or changed
    for mine, theirs in zip(big["tables"], SC.model().tables):
        n = theirs[0].size
        assert mine[0].size > n and all(np.array_equal(a[:n], b) for a, b in zip(mine[:3], theirs[:3])) and mine[3][:n].tobytes() == theirs[3].tobytes()
        assert len(set(zip(mine[0].tolist(), mine[1].tolist(), mine[2].tolist()))) == mine[0].size
    assert (1 << big["cap_log2"]) >= 2 * max(t[0].size for t in big["tables"])


def test_the_packed_steps_hold_the_models():
    m = SC.model()
    packed = m.steps("world fish")
    assert packed.shape == (9, SC.STEPS_CAP) and packed["result"]["iterations"].any() and packed["recall"]["n_edges"].any()
    n = sum(len(w["steps"]) for w in m.want["world fish"])
    assert int((packed["solve_id"] != 0).sum()) == n

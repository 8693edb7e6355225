"""tests/nlhe_translate_model.py pinned on the CPU: to the reference's own tests of Game::translate and Size::translate, to the two
facts that make Translation::Snap another function than edgify and Phargmax another than Snap, to the counter stream of the harmonic
draws, and to the two cuts of Recall::history() (the 12-edge path, MAX_RAISE_REPEATS)."""
import math

import pytest

import nlhe_aivat_model as AM
import nlhe_translate_cases as TC
import nlhe_translate_model as TM
import oracle_nlhe as ON

KINDS = ("snap", "harmonic", "phargmax")
PREF, FLOP = 0, 1


def test_snap_clamps_outside_the_opening_grid():  # kicker/src/game.rs:1903-1911
    assert TM.translate(PREF, 3, ON.Raise(2), 0, TM.SNAP, 0.0) == ON.Open(2)
    assert TM.translate(PREF, 3, ON.Raise(20), 0, TM.SNAP, 0.0) == ON.Open(5)


def test_an_opening_tie_goes_low():  # kicker/src/size.rs:444-449
    assert TM.translate(PREF, 0, ON.Raise(7), 0, TM.SNAP, 0.0) == ON.Open(3)


def test_sixty_into_a_hundred_on_the_flop_is_half_pot():  # kicker/src/size.rs:466-470
    assert TM.translate(FLOP, 100, ON.Raise(60), 0, TM.SNAP, 0.0) == ON.RaiseOdds(1, 2)
    assert TM.recall(TC.FLOP_60_INTO_100)["play_edges"][-1] == ON.RaiseOdds(1, 2)


@pytest.mark.parametrize("kind", KINDS)
def test_other_actions_pass_through(kind):  # kicker/src/game.rs:1814-1822, 1878-1898
    for action, edge in ((ON.Fold, ON.E_FOLD), (ON.Check, ON.E_CHECK), (ON.Call(1), ON.E_CALL), (ON.Shove(199), ON.E_SHOVE)):
        for u in (0.0, 0.999):
            assert TM.translate(PREF, 3, action, 0, TM.KINDS[kind], u) == edge
    got = TM.recall(TC.SINGLES["passive"], kind)
    assert got["status"] == TM.OK and got["play_edges"] == [ON.E_CALL] + [ON.E_CHECK] * 7


def test_phargmax_and_harmonic_stay_in_the_bracket():  # kicker/src/game.rs:1843-1873
    assert TM.translate(PREF, 3, ON.Raise(7), 0, TM.PHARGMAX, 0.0) in (ON.Open(3), ON.Open(4))
    assert {TM.translate(PREF, 3, ON.Raise(7), 0, TM.HARMONIC, u / 64) for u in range(64)} == {ON.Open(3), ON.Open(4)}
    for chips in (4, 6, 8, 10):  # on the grid every policy answers the anchor
        assert len({TM.translate(PREF, 3, ON.Raise(chips), 0, k, 0.5) for k in (TM.SNAP, TM.HARMONIC, TM.PHARGMAX)}) == 1


def test_snap_is_not_edgify_on_the_pot_12_line():
    game = AM._start(0, (200, 200), TC.HOLES)
    for kind, chips in TC.POT12.plays[:-1]:
        while AM._turn(game) == ON.CHANCE:
            game = AM._consume(game, ON.Draw(TC.DRAWS[AM._street(game)]))
        game = AM._consume(game, (AM.KIND[kind], chips, 0))
    game = AM._consume(game, ON.Draw(TC.DRAWS[1]))
    assert (AM._street(game), game.pot) == (2, 12)
    assert AM._edgify(game, ON.Raise(5), 0) == 11 == ON.RaiseOdds(1, 3)
    got = TM.recall(TC.POT12)
    assert got["status"] == TM.OK and got["play_edges"][-1] == 12 == ON.RaiseOdds(1, 2)
    assert got["edges"] == [ON.Open(2), ON.E_CALL, ON.E_DRAW, ON.E_CHECK, ON.E_CHECK, ON.E_DRAW, 12]
    assert 5 / 12 - 1 / 3 == 0.08333333333333337 and 1 / 2 - 5 / 12 == 0.08333333333333331


def test_the_three_bet_under_the_three_policies():
    assert TM.recall(TC.THREE_BET, "snap")["play_edges"] == [ON.Open(2), 15]
    assert TM.recall(TC.THREE_BET, "phargmax")["play_edges"] == [ON.Open(3), 18]  # the open itself: 2.5 bb, p = 3/7
    pairs = TM.lattice(PREF, 1)[1]
    assert [e for _, e in pairs] == [15, 18] and TM.bracket(pairs, 1.5) == (0, 1) and TM.pharmonic(pairs, 0, 1, 1.5) == 0.4
    for seed, hand_id in ((0, 0), (0, 77), (5, 1 << 40)):
        want = 15 if TM.uniform(seed, hand_id, 1) < 0.4 else 18
        assert TM.recall(TC.THREE_BET, "harmonic", seed=seed, hand_id=hand_id)["play_edges"][1] == want


def test_the_harmonic_frequency_over_4096_hand_ids():
    seed, n = 0, 4096
    low = [TM.recall(TC.THREE_BET, "harmonic", seed=seed, hand_id=i)["play_edges"][1] == 15 for i in range(n)]
    assert low == [TM.uniform(seed, i, 1) < 0.4 for i in range(n)]  # exactly the hands whose draw is below p
    assert abs(sum(low) / n - 0.4) <= 5 * math.sqrt(0.4 * 0.6 / n)


def test_the_draw_of_a_play_is_its_index_in_the_hand():
    us = [TM.uniform(3, 9, j) for j in range(48)]
    assert all(0.0 <= u < 1.0 for u in us) and len(set(us)) == 48
    assert TM.uniform(3, 9, 1) != TM.uniform(3, 10, 1) != TM.uniform(4, 10, 1)
    # a call before the raise moves the raise to another index, and to another draw: the draws do not depend on the content
    assert TM.uniform(0, 0, 1) == float(TM.RO.node_hash(0, 3, 0, 1) >> 11) * 2.0 ** -53


def test_raises_past_the_repeats_become_shove():
    got = TM.recall(TC.RAISE_WAR)
    assert got["status"] == TM.OK and [k for k, _ in TC.RAISE_WAR.plays] == ["raise"] * 6
    assert got["play_edges"][0] == ON.Open(2) and all(10 <= e < 20 for e in got["play_edges"][1:4])
    assert got["play_edges"][4:] == [ON.E_SHOVE, ON.E_SHOVE]  # depth 4 and 5: Edge::raises is empty
    assert got["n_choices"] > 0 and TM.PM.edges(got["choices"])[0] == ON.E_SHOVE  # and so is the head's grid


def test_the_depth_stops_at_the_twelve_edge_cap():
    got = TM.recall(TC.LONG_RIVER)
    assert got["status"] == TM.OK and len(got["edges"]) == 16
    depths = [TM.aggression(got["edges"][:k]) for k in range(17)]
    assert depths[10:13] == [0, 1, 2] and depths[12:] == [2] * 5  # the 13th edge on no longer counts
    # the fifth river raise is translated at depth 2, not 4: a grid edge, where an uncut path would answer Shove
    assert [k for k, _ in TC.LONG_RIVER.plays[7:12]] == ["raise"] * 5
    assert 10 <= got["edges"][14] < 20 and got["edges"][14] in ON.edge_raises(3, 2)
    assert got["past"] == ON.path_pack(got["edges"][9:])  # the river's seven edges
    assert TM.recall(TC.LONG_RIVER, upto=12)["n_choices"] > 0


def test_the_shared_hands_are_what_they_are_meant_to_be():
    for name, hand in TC.SINGLES.items():
        want = TM.ILLEGAL if name == "root_raise_2" else TM.OK
        assert all(TM.recall(hand, kind)["status"] == want for kind in KINDS), name
    assert TM.recall(TC.SINGLES["root_raise_20"])["play_edges"] == [ON.Open(5)]
    assert TM.recall(TC.SINGLES["root_raise_7"])["play_edges"] == [ON.Open(3)]
    run_out = TM.recall(TC.ALL_IN_RUN_OUT)
    assert run_out["edges"][-3:] == [ON.E_DRAW] * 3 and run_out["n_choices"] == 0 and run_out["draws"] == TC.DRAWS
    folded = TM.recall(TC.FOLDED)
    assert folded["status"] == TM.OK and folded["n_choices"] == 0 and folded["draws"] == (0, 0, 0)
    assert TM.recall(TC.FOLDED, pov=1)["status"] == TM.CARDS  # the unknown hole is no point of view
    for hand, pov, status in TC.refusals():
        got = TM.recall(hand, pov=pov)
        assert got["status"] == status and got["edges"] == [] and got["present"] == 0
    assert TM.recall(TC.POT12, upto=6)["status"] == TM.LENGTH
    # cut before the turn bet, the recall is at the decision at the start of the turn, the street dealt
    cut = TM.recall(TC.POT12, upto=4)
    assert cut["edges"][-1] == ON.E_DRAW and cut["past"] == 0 and cut["n_choices"] > 0 and cut["draws"] == (TC.DRAWS[0], TC.DRAWS[1], 0)
    # the two points of view differ in the hole and the bucket only
    a, b = TM.recall(TC.MULTI_STREET, pov=0), TM.recall(TC.MULTI_STREET, pov=1)
    assert a["edges"] == b["edges"] and a["hole"] != b["hole"] and a["present"] != b["present"]

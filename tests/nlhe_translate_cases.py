"""The hands the translation tests share (helper, no tests): lines played through the CPU oracle's rules engine into AivatHands, the
single-hand cases of the contract, one hand per status, and the model's answers as the arrays the library writes.
tests/test_nlhe_translate_model.py pins the model on them; tests/test_gpu_nlhe_translate.py compares rp_nlhe_translate with it."""
import ctypes as C

import numpy as np

import nlhe_aivat_model as AM
import nlhe_translate_model as TM
import oracle_nlhe as ON
from robopoker_amd.nlhe import MAX_PLAYS, RECALL_DTYPE, AivatHand

HOLES = (0b11 << 50, 0b11 << 10)
DRAWS = (0b111 << 20, 1 << 30, 1 << 31)
KIND_NAME = {ON.FOLD: "fold", ON.CALL: "call", ON.CHECK: "check", ON.RAISE: "raise", ON.SHOVE: "shove"}


def line(script, dealer=0, stacks=(0, 0), holes=HOLES, draws=DRAWS, seat=0):
    """an AivatHand from a script played on the real game, streets dealt from `draws` as they come due: "x" check, "c" call, "f" fold,
    "s" shove, "r" the minimum raise, an integer a raise of that many chips (illegal ones are recorded as they are)"""
    game = AM._start(dealer, stacks if tuple(stacks) != (0, 0) else (ON.STACK, ON.STACK), holes)
    o, plays = ON.lib(), []
    amount = lambda name: o.ora_nlhe_amount(C.byref(game), ON.AMOUNT[name])  # noqa: E731
    for step in script:
        while AM._turn(game) == ON.CHANCE:
            game = AM._consume(game, ON.Draw(draws[AM._street(game)]))
        a = {"x": lambda: ON.Check, "f": lambda: ON.Fold, "c": lambda: ON.Call(amount("to_call")), "s": lambda: ON.Shove(amount("to_shove")),
             "r": lambda: ON.Raise(amount("to_raise"))}.get(step, lambda: ON.Raise(step))()
        plays.append((KIND_NAME[a[0]], a[1]))
        if AM._allowed(game, a):
            game = AM._consume(game, a)
    while AM._turn(game) == ON.CHANCE:  # the run-out, or the street the last play closed
        game = AM._consume(game, ON.Draw(draws[AM._street(game)]))
    n_streets = AM._street(game)
    return AivatHand(holes, draws[:n_streets], plays, seat=seat, stacks=stacks, dealer=dealer)


POT12 = line([5, "c", "x", "x", 5])  # Snap 12 where edgify gives 11
THREE_BET = line([5, 12])  # x = 1.5 between 1:1 and 2:1: Snap 15, Phargmax 18, Harmonic 15 with probability 0.4
FLOP_60_INTO_100 = line([49, "c", "x", 60])
RAISE_WAR = line([5, "r", "r", "r", "r", "r"])  # the fifth and sixth raise meet an empty grid
# 9 edges to the river, a check, then raises: the path is full after the second raise
LONG_RIVER = line(["r", "c", "x", "x", "x", "x", "x", "r", "r", "r", "r", "r", "c"])
MULTI_STREET = line([6, "c", "x", 5, 17, "c", 20, "c", "x", "x"], dealer=1, seat=1)
ALL_IN_RUN_OUT = line([5, "s", "s"], stacks=(45, 45))  # the board runs out after the last play
LONE_BETTOR = line([5, "s", "c"], stacks=(60, 45))  # one seat all-in and called: the flop is dealt and the other seat is asked
FOLDED = AivatHand((HOLES[0], 0), (), [("raise", 7), ("fold", 0)])  # the other seat's cards are unknown
SINGLES = dict(root_raise_2=line([2]), root_raise_20=line([20]), root_raise_7=line([7]), flop_60_into_100=FLOP_60_INTO_100, pot12=POT12,
               three_bet=THREE_BET, raise_war=RAISE_WAR, long_river=LONG_RIVER, multi_street=MULTI_STREET, all_in_run_out=ALL_IN_RUN_OUT, lone_bettor=LONE_BETTOR,
               folded=FOLDED, passive=line(["c", "x", "x", "x", "x", "x", "x", "x"]), shove_shove=line(["s", "s"]))


def refusals():
    """[(hand, pov or None, the status it is refused with)]: one per status value the entry point can answer without tables"""
    many = ["r", "c"] + ["x", "x"] + ["x", "x"] + ["x"] + ["r"] * 39  # 46 plays and three Draws: 49 edges
    return [(AivatHand(HOLES, DRAWS[:1], POT12.plays), None, TM.DRAW),  # the turn is missing
            (line([5, 6]), None, TM.ILLEGAL),  # a raise below the minimum
            (AivatHand(HOLES, (), [("raise", 5), ("fold", 0), ("check", 0)]), None, TM.ILLEGAL),  # a play after the end
            (line(many, stacks=(400, 400)), None, TM.LENGTH),
            (POT12, 2, TM.SEAT),
            (AivatHand((HOLES[0], 1 << 50 | 1 << 9), DRAWS, POT12.plays), None, TM.CARDS),  # the holes share a card
            (AivatHand(HOLES, (), [("raise", 5), (6, 0)]), None, TM.EDGE)]


def pack(answers):
    """the model's answers as the arrays rp_nlhe_translate writes"""
    n = len(answers)
    out = dict(recalls=np.zeros(n, RECALL_DTYPE), play_edges=np.zeros((n, MAX_PLAYS), np.uint8), past=np.zeros(n, np.uint64),
               present=np.zeros(n, np.uint32), choices=np.zeros(n, np.uint64), n_choices=np.zeros(n, np.uint8), status=np.zeros(n, np.uint8))
    for i, a in enumerate(answers):
        r = out["recalls"][i]
        r["hole"], r["draws"], r["stacks"], r["pov"], r["dealer"] = a["hole"], a["draws"], a["stacks"], a["pov"], a["dealer"]
        r["n_edges"] = len(a["edges"])
        r["edges"][: len(a["edges"])] = a["edges"]
        out["play_edges"][i, : len(a["play_edges"])] = a["play_edges"]
        for k in ("past", "present", "choices", "n_choices", "status"):
            out[k][i] = a[k]
    return out


def hands_of(records):
    """AIVAT_DTYPE records (a match's) -> AivatHands the model reads"""
    return [AivatHand(tuple(int(x) for x in r["hole"]), tuple(int(x) for x in r["draws"]),
                      [(int(k), int(c)) for k, c in zip(r["kind"][: r["n_plays"]], r["chips"][: r["n_plays"]])], seat=int(r["seat"]),
                      stacks=tuple(int(x) for x in r["stacks"]), dealer=int(r["dealer"]), board_mode=int(r["board_mode"])) for r in records]

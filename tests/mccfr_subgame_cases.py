"""Entries, beliefs and blueprints for the table-game subgame tests (helper, no tests): the smallest shapes at which
rp_mccfr_subgame_solve can go wrong, shared by the model's CPU tests and the device's parity tests."""
from __future__ import annotations

import numpy as np

import mccfr_subgame_model as M
from robopoker_amd import _lib, games
from robopoker_amd.mccfr import ENC_DTYPE, SUBGAME_ENTRY_DTYPE, SUBGAME_PRIOR_DTYPE

ITERATIONS = (1, 2, 7, 64)
CHECK, BET, FOLD, CALL = 0, 1, 0, 1  # slots: [Check, Bet | Raise] at an open or checked spot, [Fold, Call] facing a bet

# (label, holes, prefix, external, reach): the entries of the reference's tests and the tree shapes around them
KUHN = [("root", (4, 1), (), 1, False), ("after check", (0, 3), (CHECK,), 0, False), ("after bet", (2, 5), (BET,), 0, False),
        ("check-bet, reach", (1, 4), (CHECK, BET), 1, True), ("terminal observed", (0, 2), (CHECK, CHECK), 1, False)]
LEDUC = [("root", (4, 1), (), 1, False), ("after check: the walker's child is the board deal", (0, 3), (CHECK,), 0, False),
         ("after raise", (2, 5), (BET,), 0, False), ("check-raise, reach", (1, 4), (CHECK, BET), 1, True),
         ("round 2: to the terminals", (0, 3), (CHECK, CHECK, ("board", 4)), 0, False),
         ("round 2 after a raise, P1 to act", (5, 2), (BET, CALL, ("board", 0), CHECK), 0, False),
         ("chance observed", (0, 2), (CHECK, CHECK), 1, False)]


def with_belief(entry, b):
    e = entry.copy()
    e["world_of"], e["weights"] = b["world_of"], b["weights"]
    return e


def variants(table, bp, prior, entry, full):
    """[(label, entry record)]: the entry under the beliefs the issue lists; `full` adds the degenerate beliefs"""
    out = []
    for W in (1, 2, 4):
        p, e = prior.copy(), entry.copy()
        p["n_worlds"] = e["n_worlds"] = W
        out.append((f"W={W}", with_belief(e, M.belief(table, bp, p))))
    if full:
        base = out[1][1]
        zero = base.copy()
        zero["weights"] = 0
        none = base.copy()
        none["world_of"] = _lib.RP_WORLD_NONE
        lone = base.copy()  # every secret in world 0, half of the weight on world 1: the iterations that draw it fall back
        lone["world_of"] = np.where(base["world_of"] == _lib.RP_WORLD_NONE, _lib.RP_WORLD_NONE, 0)
        lone["weights"] = (0.5, 0.5, 0, 0)
        empty = base.copy()
        empty["n_candidates"] = 0
        out += [("all weights zero", zero), ("no members", none), ("a world without a member", lone), ("no candidates", empty)]
    return out


def builtin_cases(game, table, bp):
    """[(label, entry record)] for the built-in Kuhn / Leduc / wide Leduc"""
    spec = KUHN if game.kind == "kuhn" else LEDUC
    out = []
    for i, (label, holes, prefix, external, reach) in enumerate(spec):
        prior, entry = games.subgame_entry(game, holes, prefix, external, reach)
        out += [(f"{label}, {v}", e) for v, e in variants(table, bp, prior[0], entry[0], full=i == 0)]
    return out


def custom_cases(table, bp):
    """tests/game_tables.py "chance16_mid": deal 0 (3), deal 1 (3), act 0 (2), chance (16), act 1 (3 actions), act 0 (2).  The other
    seat's secret is its deal; the candidates are the states that differ in it."""
    def state(k0, k1, path):
        s = table.kids[table.kids[0][k0]][k1]
        for slot in path:
            s = table.kids[s][slot]
        return s

    out = []
    for label, (k0, k1), path, external in (("root: both children are chance leaves", (1, 2), (), 1), ("three actions", (2, 0), (1, 5), 0),
                                            ("last decision", (0, 1), (0, 15, 2), 1)):
        prior, entry = np.zeros(1, SUBGAME_PRIOR_DTYPE)[0], np.zeros(1, SUBGAME_ENTRY_DTYPE)[0]
        cands = [state(*((k0, k) if external == 1 else (k, k1)), path) for k in range(3)]
        prior["n_prior"], prior["internal"], prior["mode"], prior["n_path"] = 3, 1 - external, 1, len(path)
        prior["root_state"][:3] = [state(*((k0, k) if external == 1 else (k, k1)), ()) for k in range(3)]
        prior["path"][:len(path)], prior["secret"][:3] = path, (0, 1, 2)
        entry["observed"], entry["external"], entry["n_candidates"], entry["harvest_info"] = state(k0, k1, path), external, 3, _lib.RP_NO_INFO
        entry["candidate"][:3], entry["secret"][:3], entry["harvest_order"] = cands, (0, 1, 2), [2, 0, 1] + list(range(3, 16))
        if table.actions[table.info[int(entry["observed"])]] == 2:
            entry["harvest_order"][:3] = (1, 0, 2)
        out += [(f"{label}, {v}", e) for v, e in variants(table, bp, prior, entry, full=False)]
    return out


def malformed(entry, table):
    """[(status, entry record)]: one broken field each"""
    def broken(**fields):
        e = entry.copy()
        for k, v in fields.items():
            if isinstance(v, tuple):
                e[k][v[0]] = v[1]
            else:
                e[k] = v
        return e

    return [(M.STATE, broken(observed=table.n_states)), (M.STATE, broken(candidate=(1, 0xFFFFFFFF))), (M.SECRET, broken(secret=(0, 16))),
            (M.WORLDS, broken(n_worlds=0)), (M.WORLDS, broken(n_worlds=5)), (M.WEIGHT, broken(weights=(1, np.nan))),
            (M.WEIGHT, broken(weights=(0, -1.0))), (M.ORDER, broken(harvest_order=(0, 15))), (M.INFO, broken(harvest_info=table.n_infos)),
            (M.SEAT, broken(external=2)), (M.COUNT, broken(n_candidates=17))]


def corner_rows(table, seed=7):
    """a blueprint of corner values for rp_mccfr_import: zero and subnormal weights, negative regrets, garbage past an infoset's actions"""
    rng = np.random.default_rng(seed)
    rows = np.zeros((table.n_infos, table.A), ENC_DTYPE)
    rows["weight"] = rng.choice(np.array([0.0, 1e-39, 1.0, 3.5, 1e12], np.float32), rows.shape)
    rows["regret"] = rng.choice(np.array([-3.0, 0.0, 2.5, 40.0], np.float32), rows.shape)
    rows["payoff"] = rng.choice(np.array([-1.5, 0.0, 2.5, 7.25], np.float32), rows.shape)
    rows["visits"] = rng.choice(np.array([0, 3, 11, 0xFFFFFFFF], np.uint32), rows.shape)
    return rows.reshape(-1)


def stack(cases):
    return np.array([e for _, e in cases], SUBGAME_ENTRY_DTYPE)

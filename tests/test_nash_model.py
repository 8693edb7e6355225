"""tests/mccfr_nash_model.py against the CPU oracle: after three oracle steps the model's exploitability is ora_mccfr_exploitability's,
bit for bit, on the four built-in games and every caller-built table of the catalogue.  This pins the model without a GPU, so what
tests/test_gpu_nash.py asserts about `choice` and `cfv` (which the oracle does not expose) rests on something checked."""
import numpy as np
import pytest

import game_tables as GT
import mccfr_nash_model as M
import oracle
from robopoker_amd.games import Game

BUILTIN = ["kuhn", "leduc", "rps", "leduc_wide"]


def the_game(name):
    return Game(name) if name in BUILTIN else GT.game(name)


@pytest.mark.parametrize("name", BUILTIN + list(GT.CATALOGUE))
def test_model_exploitability_is_the_oracles(name):
    g = the_game(name)
    ora = oracle.OracleSolver(g, "linear", "linear", "external", batch=130, seed=5)
    for _ in range(3):
        ora.step()
    got = M.best_response(g.table, ora.export())
    want = np.float32(ora.exploitability())
    assert not np.isnan(want)
    assert got["exploitability"].view(np.uint32) == want.view(np.uint32), (name, float(got["exploitability"]), float(want))
    # the parts hang together: the scalar is the mean of the values, every choice is an action of its infoset
    assert got["values"].shape == (g.table.n_players,)
    assert all(got["choice"][i] < g.n_actions(i) for i in range(g.n_infos))


@pytest.mark.parametrize("name", ["one_player", "chance16_mid", "nodes62"])
def test_model_on_an_empty_table_finds_ties(name):
    # epoch 0: every weight 0, avg uniform through EPS.  These tables have cells that tie exactly (payoffs are multiples of 0.25), and the
    # last maximum must win; rock-paper-scissors (asymmetric payoffs here) and Kuhn have no exact tie on an empty table
    g = the_game(name)
    ora = oracle.OracleSolver(g, "linear", "linear", "external", batch=1, seed=0)
    got = M.best_response(g.table, ora.export())
    assert got["ties"] > 0
    assert got["exploitability"].view(np.uint32) == np.float32(ora.exploitability()).view(np.uint32)

"""The numpy model of the three distributions (tests/nlhe_policy_model.py) equals the CPU oracle's ora_mccfr_policy bit for bit:
every Leduc infoset, all three kinds, after 200 oracle steps — with the default hyperparameters and with others.  The GPU tests of
the policy queries (tests/test_gpu_nlhe_policy.py) compare against this model."""
import numpy as np
import pytest

import nlhe_policy_model as PM
from oracle import OracleSolver
from robopoker_amd import Game
from robopoker_amd.mccfr import default_hyper


def _hyper(custom):
    hp = default_hyper()
    if custom:
        hp.temperature, hp.smoothing, hp.curiosity = 0.7, 1.5, 0.1
    return hp


@pytest.mark.parametrize("custom", [False, True], ids=["default_hyper", "tau0.7_beta1.5_eps0.1"])
def test_model_equals_the_oracle_on_every_leduc_infoset(custom):
    game = Game("leduc")
    hp = _hyper(custom)
    ora = OracleSolver(game, regret="linear", weight="linear", batch=16, seed=3, hyper=hp)
    for _ in range(200):
        ora.step()
    rows = ora.export().reshape(game.n_infos, game.max_actions)
    assert np.count_nonzero(rows["weight"]) > game.n_infos  # the table is trained, not the initial one
    for info in range(game.n_infos):
        n = game.n_actions(info)
        for kind in ("iterated", "averaged", "sampling"):
            want = ora.policy(info, kind)
            values = rows[info]["regret"] if kind == "iterated" else rows[info]["weight"]
            got = PM.distribution(kind, values, n, hp.temperature, hp.smoothing, hp.curiosity)
            assert np.array_equal(got[:n].view(np.uint32), want.view(np.uint32)), (info, kind, got[:n], want)
            assert not got[n:].any()


def test_choices_decoding_and_default_regrets():
    path = 2 | (4 << 5) | (12 << 10)  # FOLD, CALL, a raise, then a gap
    assert PM.nch(path) == 3 and list(PM.edges(path)) == [2, 4, 12, 0, 0, 0, 0, 0, 0]
    assert PM.nch(path | (5 << 20)) == 3  # a group behind a zero group is not part of the path
    assert PM.nch(0) == 0 and PM.nch((1 << 64) - 1) == 9
    assert [float(PM.default_regret(e)) for e in (2, 3, 4, 5, 6, 15)] == [100.0, 50.0, 50.0, 0.0, 10.0, 10.0]

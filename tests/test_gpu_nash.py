"""The best response on the device (csrc/mccfr_nash.hpp: rp_mccfr_exploitability_device, rp_mccfr_best_response, rp_mccfr_solve_to)
against the host path of the library, the CPU oracle and tests/mccfr_nash_model.py — bit for bit, in both launch shapes.

The oracle gives the scalar only; `values`, `choice` and `cfv` are compared with the numpy model, which tests/test_nash_model.py pins
to the oracle on the CPU.  RP_NASH_VARIANT is read when a handle builds its tree, i.e. by its first best-response call.

Ties: the issue behind these tests expected exact ties in rock-paper-scissors and Kuhn on an empty table.  There are none: this
library's RPS pays asymmetrically (cfv 1/3, -1/3, 0 at epoch 0) and no Kuhn infoset has two equal cells (model and oracle agree on
both, tests/test_nash_model.py).  Both games stay in the tie test for their choices; the games that do tie on an empty table
(one_player 4 cells, chance16_mid 7, nodes62 15 over 14 actions) are added and carry the assertion that the case is not vacuous.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import game_tables as GT
import mccfr_nash_model as M
import oracle
from robopoker_amd import _lib
from robopoker_amd.games import Game
from robopoker_amd.mccfr import Solver

pytestmark = pytest.mark.gpu

BUILTIN = ["kuhn", "leduc", "rps", "leduc_wide"]
SCALAR = BUILTIN + [n for n in GT.CATALOGUE if n != "infos8191"]
PARTS = ["leduc", "three_players_a5", "widest_a16", "one_player", "two_states", "chance16_mid"]
VARIANTS = ["one", "levels"]
ONE_LDS_BYTES = 64 * 1024  # NASH_ONE_LDS_BYTES (csrc/mccfr_nash.hpp, include/rp_mi355x.h)


@functools.lru_cache(maxsize=None)
def the_game(name):
    """one object per game for the whole module: a table's pointers live as long as its Game"""
    return Game(name) if name in BUILTIN else GT.game(name)


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def oracle_after(name, steps=5):
    """the oracle's table and exploitability after `steps` ordered steps (batch 130, linear / linear / external, seed 31), once per game"""
    ora = oracle.OracleSolver(the_game(name), "linear", "linear", "external", batch=130, seed=31)
    for _ in range(steps):
        ora.step()
    rows = ora.export()
    rows.setflags(write=False)
    return rows, np.float32(ora.exploitability())


@functools.lru_cache(maxsize=None)
def model_after(name):
    return M.best_response(the_game(name).table, oracle_after(name)[0])


def device_after(name, steps=5):
    dev = Solver(the_game(name), "linear", "linear", "external", batch=130, seed=31)
    dev.step_async(steps)
    dev.sync()
    return dev


def device_value(dev):
    """one rp_mccfr_exploitability_device into a device word, read back after a sync"""
    buf = torch.zeros(1, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()  # the fill runs on torch's stream, the call on the solver's
    dev.exploitability_device(buf.data_ptr())
    dev.sync()
    return np.float32(buf.cpu().numpy()[0])


def working_set_bytes(g):
    return 4 * (M.Tree(g.table).n + 2 * g.n_infos * g.max_actions + g.n_infos)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", SCALAR)
def test_scalar_is_the_hosts_and_the_oracles_in_both_shapes(gpu, monkeypatch, name, variant):
    monkeypatch.setenv("RP_NASH_VARIANT", variant)
    rows, want = oracle_after(name)
    dev = device_after(name)
    got = device_value(dev)
    assert dev.nash_variant() == variant
    host = np.float32(dev.exploitability())
    print(name, variant, float(got), float(host), float(want))
    assert bits(got) == bits(host)
    assert bits(host) == bits(want)
    assert not np.isnan(got)
    if name == "two_states":
        assert got < 0  # a player root over one terminal: nothing to exploit, the payoffs are not zero-sum


@pytest.mark.parametrize("name,variant", [("leduc", "one"), ("leduc_wide", "levels")])
def test_unforced_shape(gpu, monkeypatch, name, variant):
    monkeypatch.delenv("RP_NASH_VARIANT", raising=False)
    dev = device_after(name, steps=1)
    assert dev.nash_variant() == variant


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", PARTS)
def test_parts_are_the_models(gpu, monkeypatch, name, variant):
    monkeypatch.setenv("RP_NASH_VARIANT", variant)
    dev = device_after(name)
    assert np.array_equal(bits(dev.export()["weight"]), bits(oracle_after(name)[0]["weight"]))  # the model's input is this table
    want = model_after(name)
    got = dev.best_response()
    assert dev.nash_variant() == variant
    assert bits(got["exploitability"]) == bits(want["exploitability"])
    assert np.array_equal(bits(got["values"]), bits(want["values"]))
    assert np.array_equal(got["choice"], want["choice"])
    assert got["cfv"].shape == want["cfv"].shape and np.array_equal(bits(got["cfv"]), bits(want["cfv"]))
    # any output may be NULL
    e = np.zeros(1, dtype=np.float32)
    _lib.check(dev._lib.rp_mccfr_best_response(dev._h, e.ctypes.data_as(C.POINTER(C.c_float)), None, None, None))
    assert bits(e[0]) == bits(want["exploitability"])


TIED = {"one_player", "chance16_mid", "nodes62"}  # exact ties on an empty table; rps and kuhn have none (module docstring)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["rps", "kuhn", "one_player", "chance16_mid", "nodes62"])
def test_ties_keep_the_last_maximum(gpu, monkeypatch, name, variant):
    # a fresh handle: epoch 0, every weight 0, avg uniform through EPS
    monkeypatch.setenv("RP_NASH_VARIANT", variant)
    g = the_game(name)
    dev = Solver(g, "linear", "linear", "external", batch=1, seed=0)
    want = M.best_response(g.table, dev.export())
    if name in TIED:
        assert want["ties"] > 0
    got = dev.best_response()
    assert np.array_equal(got["choice"], want["choice"])
    assert np.array_equal(bits(got["cfv"]), bits(want["cfv"]))
    assert bits(got["exploitability"]) == bits(want["exploitability"])


def test_stream_order_and_staleness(gpu, monkeypatch):
    monkeypatch.delenv("RP_NASH_VARIANT", raising=False)
    g = the_game("leduc")
    dev = Solver(g, "linear", "linear", "external", batch=600, seed=11, mode="composed")
    ora = oracle.OracleSolver(g, "linear", "linear", "external", batch=600, seed=11)
    buf = torch.zeros(2, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    # queued back to back, one sync at the end: each value is of the tables as the stream had left them
    dev.exploitability_device(buf.data_ptr())
    dev.step_async(3)
    dev.exploitability_device(buf.data_ptr() + 4)
    dev.sync()
    e0 = np.float32(ora.exploitability())
    for _ in range(3):
        ora.step_world(1)
    e3 = np.float32(ora.exploitability())
    got = buf.cpu().numpy()
    assert bits(e0) != bits(e3)
    assert bits(got[0]) == bits(e0) and bits(got[1]) == bits(e3)
    # another solver's table through load_rows, then a single set: the next call sees each
    other = oracle.OracleSolver(g, "floored", "linear", "external", batch=130, seed=99)
    for _ in range(2):
        other.step()
    rows = other.export()
    dev.load_rows(rows, other.epoch)
    want = M.best_response(g.table, rows)
    assert bits(want["exploitability"]) != bits(e3)
    assert bits(device_value(dev)) == bits(want["exploitability"])
    info = int(np.argmax(rows["weight"].reshape(g.n_infos, g.max_actions)[:, 0] > 0))
    dev.set(info, 0, weight=1000.0, regret=0.0, payoff=0.0, visits=1)
    want2 = M.best_response(g.table, dev.export())
    assert bits(want2["exploitability"]) != bits(want["exploitability"])
    assert bits(device_value(dev)) == bits(want2["exploitability"])


def oracle_solve_to(ora, target, check_every, max_steps):
    """the loop of rp_mccfr_solve_to over the oracle: (steps, last value, reached, number of checks)"""
    steps = checks = 0
    while True:
        n = min(check_every, max_steps - steps)
        for _ in range(n):
            ora.step()
        steps += n
        checks += 1
        e = np.float32(ora.exploitability())
        if e < np.float32(target):
            return steps, e, True, checks
        if steps >= max_steps:
            return steps, e, False, checks


def assert_same_tables(dev, ora):
    a, b = dev.export(), ora.export()
    for f in ("visits", "regret", "weight", "payoff"):
        assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), f
    assert dev.epoch == ora.epoch and dev.counters() == ora.counters()


@pytest.mark.parametrize("name,batch,check_every,target", [("leduc", 128, 4, 0.5), ("kuhn", 64, 2, 0.1)])
def test_solve_to_stops_at_the_first_check_under_the_target(gpu, monkeypatch, name, batch, check_every, target):
    monkeypatch.delenv("RP_NASH_VARIANT", raising=False)
    g = the_game(name)
    dev = Solver(g, "floored", "linear", "external", batch=batch, seed=7)
    ora = oracle.OracleSolver(g, "floored", "linear", "external", batch=batch, seed=7)
    want_steps, want_e, want_hit, checks = oracle_solve_to(ora, target, check_every, 400)
    print(name, want_steps, float(want_e), checks)
    assert want_hit and checks > 1  # not at the first check
    steps, e, hit = dev.solve_to(target, check_every, 400)
    assert (steps, hit) == (want_steps, True)
    assert bits(e) == bits(want_e)
    assert_same_tables(dev, ora)


def test_solve_to_runs_out_of_steps_on_a_short_last_block(gpu, monkeypatch):
    monkeypatch.delenv("RP_NASH_VARIANT", raising=False)
    g = the_game("leduc")
    dev = Solver(g, "floored", "linear", "external", batch=128, seed=7)
    ora = oracle.OracleSolver(g, "floored", "linear", "external", batch=128, seed=7)
    want_steps, want_e, want_hit, checks = oracle_solve_to(ora, 0.5, 4, 6)
    assert (want_steps, want_hit, checks) == (6, False, 2)
    steps, e, hit = dev.solve_to(0.5, 4, 6)
    assert (steps, hit) == (6, False)
    assert bits(e) == bits(want_e)
    assert_same_tables(dev, ora)


def test_the_limit_of_the_one_workgroup_shape(gpu, monkeypatch):
    # unforced: the largest game under the documented working set of k_nash_one's LDS and the smallest over it
    monkeypatch.delenv("RP_NASH_VARIANT", raising=False)
    sizes = {n: working_set_bytes(the_game(n)) for n in BUILTIN + list(GT.CATALOGUE)}
    under = max((n for n in sizes if sizes[n] <= ONE_LDS_BYTES), key=sizes.get)
    over = min((n for n in sizes if sizes[n] > ONE_LDS_BYTES), key=sizes.get)
    print(under, sizes[under], over, sizes[over])
    assert sizes[under] > ONE_LDS_BYTES * 3 // 4  # the pair is about the limit, not about two sizes far from it
    for name, variant in ((under, "one"), (over, "levels")):
        dev = device_after(name, steps=2)
        assert dev.nash_variant() == variant
        assert bits(device_value(dev)) == bits(oracle_after(name, 2)[1])

"""The unit-slab path of k_fold_groups on a machine without a GPU: a selection of tests/test_gpu_mccfr_unit_fold.py through the wave64
execution model of tests/emul/ (guard pages and the trap on: a load or a store outside a buffer fails the run).  One block, two
blocks, a second group of one tree, Kuhn and Leduc, the three schedules (two unit ones and the mixed one, which takes the general
path), against the oracle bit for bit; a resumed table and overflowing regret deltas, split against the one-launch fold.  Test
infrastructure, as tests/test_emul.py; nothing here is a measurement."""
from __future__ import annotations

import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get("RP_EMUL_CXX", "/opt/rocm/lib/llvm/bin/clang++")

EXPR = ("(test_unit_fold_equals_the_oracle and (-1] or -257] or -16385])) or test_unit_fold_on_a_resumed_table "
        "or test_overflowing_regret_deltas_split_equals_fused")


@pytest.fixture(scope="module")
def emulated_library():
    if not os.path.exists(CLANG):
        pytest.skip(f"{CLANG} (host compiler of the execution model) is not installed")
    sys.path.insert(0, os.path.join(ROOT, "tests", "emul"))
    import build as emul_build

    return emul_build.build(jobs=os.cpu_count() or 4)


def test_unit_fold_under_the_wave64_model(emulated_library):
    env = dict(os.environ, RP_EMUL="1", RP_EMUL_GUARD="1", RP_EMUL_TRAP="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_mccfr_unit_fold.py", "-m", "gpu", "-q", "-x", "-k", EXPR,
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "24 passed" in r.stdout and " failed" not in r.stdout, tail  # 2 games x 3 schedules x 3 batches, 4 resumed, 2 overflowing

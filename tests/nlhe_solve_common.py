"""What the tests of the two re-solves (tests/test_gpu_nlhe_depth.py, tests/test_gpu_nlhe_subgame.py) and scripts/nlhe_subgame_rate.py
share: card masks, float bit patterns, and the exported blueprint as the models read it.  A plain module, imported by name."""
import numpy as np


def cards(*cs):
    return sum(1 << c for c in cs)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


class Table:
    """the exported blueprint as the model reads it"""

    def __init__(self, past, present, choices, enc):
        self.rows = {(int(p), int(q), int(c)): enc[i] for i, (p, q, c) in enumerate(zip(past, present, choices))}

    def enc(self, key):
        return self.rows.get(key)

    def get(self, key):
        row = self.rows.get(key)
        return None if row is None else row["weight"]

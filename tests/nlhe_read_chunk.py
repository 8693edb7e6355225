"""The launch-chunk knob of the NLHE read side for the cut-invariance tests (helper, no tests).  Every batched read-side call cuts its
batch into launches of at most 2^20 items and rebuilds each launch's arguments from the base pointers (`rp::chunks` in
robopoker_amd/csrc/nlmc.hip); RP_NLHE_READ_CHUNK, read at every call, makes the launches small enough for a batch of a few items to
need several.  The reference of every comparison is the same call with the variable unset: one launch."""
import contextlib
import os

ENV = "RP_NLHE_READ_CHUNK"


@contextlib.contextmanager
def read_chunk(value):
    """the variable at `value` (None: unset) inside the block, as it was before after it"""
    saved = os.environ.pop(ENV, None)
    try:
        if value is not None:
            os.environ[ENV] = str(value)
        yield
    finally:
        os.environ.pop(ENV, None)
        if saved is not None:
            os.environ[ENV] = saved


def cuts(n):
    """launches of one item, an odd cut, a last launch of one item, one launch through the knob's code path"""
    assert n >= 7
    return (1, 3, n - 1, n)


def same(got, want, what):
    """two answers (dicts or sequences of arrays) byte for byte"""
    keys = list(want) if isinstance(want, dict) else range(len(want))
    for k in keys:
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (what, k)


def tail(answer, start):
    """the items of an answer from `start` on"""
    return {k: v[start:] for k, v in answer.items()} if isinstance(answer, dict) else [v[start:] for v in answer]

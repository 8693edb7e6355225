"""The model the policy-query tests compare against (helper, no tests): the three distributions of a profile row in numpy with an
explicit float32 left fold (one rounding per operation), the decoding of a choices Path, the default regrets of an absent
infoset and the table's key hash, restated from include/rp_mi355x.h (rp_nlhe_policy) and csrc/nlmc_common.hpp.

tests/test_nlhe_policy_model.py pins the distributions to the CPU oracle (ora_mccfr_policy) bit for bit."""
from __future__ import annotations

import numpy as np

A = 9
EPSILON = np.float32(1.17549435e-38)  # RP_EPSILON = f32::MIN_POSITIVE
F = np.float32
M64 = (1 << 64) - 1


def nch(choices: int) -> int:
    """consecutive non-zero 5-bit groups from bit 0, at most 9"""
    n = 0
    while n < A and (int(choices) >> (5 * n)) & 31:
        n += 1
    return n


def edges(choices: int) -> np.ndarray:
    out = np.zeros(A, np.uint8)
    for a in range(nch(choices)):
        out[a] = (int(choices) >> (5 * a)) & 31
    return out


def default_regret(edge: int) -> np.float32:
    """kicker/src/edge.rs:61-72 with BiasHyperParams::default: FOLD 2, CHECK 3, CALL 4, SHOVE 5, everything else a raise"""
    return F({2: 100.0, 3: 50.0, 4: 50.0, 5: 0.0}.get(int(edge), 10.0))


def _mix64(z: int) -> int:
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key_hash(past: int, choices: int, present: int) -> int:
    """nl_key_hash"""
    return _mix64(_mix64(int(past) ^ 0x9E3779B97F4A7C15) ^ _mix64((int(choices) + 0xD1342543DE82EF95) & M64)
                  ^ ((int(present) * 0xAF251AF3B0F025B5) & M64))


def distribution_rows(kind: str, values, n, temperature=1.0, smoothing=2.0, curiosity=0.05) -> np.ndarray:
    """values [m][A']: each row's regrets (kind "iterated") or weights ("averaged", "sampling"); n [m]: its actions.  -> float32
    [m][A'], zero from slot n[i] on.  The fold runs over the slots in order; every numpy operation below is one float32 operation
    per row, rounded on its own."""
    v = np.maximum(np.asarray(values, dtype=np.float32), EPSILON)
    n = np.asarray(n).astype(np.int64)
    m, width = v.shape
    live = np.arange(width)[None, :] < n[:, None]
    tau, beta, eps_c = F(temperature), F(smoothing), F(curiosity)
    out = np.zeros((m, width), np.float32)
    with np.errstate(all="ignore"):
        total = np.zeros(m, np.float32)
        for a in range(width):
            total = np.where(live[:, a], total + v[:, a], total)
        if kind in ("iterated", "averaged"):
            for a in range(width):
                out[:, a] = np.where(live[:, a], v[:, a] / total, F(0.0))
            return out
        assert kind == "sampling"
        denom = total + beta
        z = np.zeros(m, np.float32)
        raw = np.zeros((m, width), np.float32)
        for a in range(width):
            raw[:, a] = np.maximum((v[:, a] / tau + beta) / denom, eps_c)
            z = np.where(live[:, a], z + raw[:, a], z)
        for a in range(width):
            out[:, a] = np.where(live[:, a], raw[:, a] / z, F(0.0))
    assert out.dtype == np.float32 and total.dtype == np.float32
    return out


def distribution(kind: str, values, n: int, temperature=1.0, smoothing=2.0, curiosity=0.05) -> np.ndarray:
    """one row of distribution_rows"""
    return distribution_rows(kind, np.asarray(values, np.float32)[None, :], [n], temperature, smoothing, curiosity)[0]


def nch_rows(choices) -> np.ndarray:
    c = np.asarray(choices, dtype=np.uint64)
    n = np.zeros(c.shape, np.int64)
    for a in range(A):
        n += (n == a) & (((c >> np.uint64(5 * a)) & np.uint64(31)) != 0)
    return n.astype(np.uint8)


def edges_rows(choices) -> np.ndarray:
    c = np.asarray(choices, dtype=np.uint64)
    n = nch_rows(c)
    e = np.stack([((c >> np.uint64(5 * a)) & np.uint64(31)).astype(np.uint8) for a in range(A)], axis=1)
    return np.where(np.arange(A)[None, :] < n[:, None], e, 0).astype(np.uint8)


def default_regret_rows(e) -> np.ndarray:
    e = np.asarray(e)
    return np.select([e == 2, (e == 3) | (e == 4), e == 5], [F(100.0), F(50.0), F(0.0)], F(10.0)).astype(np.float32)


def memory_rows(choices, enc, found) -> np.ndarray:
    """what a memory query returns for m infosets: enc [m][9] their stored Encounters (ignored where found is False); the stored slots
    below nch (or the default row of an absent infoset), zero beyond"""
    e = edges_rows(choices)
    live = np.arange(A)[None, :] < nch_rows(choices)[:, None]
    found = np.asarray(found, bool)[:, None]
    out = np.zeros(enc.shape, dtype=enc.dtype)
    for f in ("weight", "payoff", "visits"):
        out[f] = np.where(live & found, enc[f], 0)
    out["regret"] = np.where(live, np.where(found, enc["regret"], default_regret_rows(e)), F(0.0))
    return out


def policy_rows(kind: str, choices, enc, found, **hyper) -> np.ndarray:
    """what a policy query returns for m infosets (arguments as memory_rows)"""
    mem = memory_rows(choices, enc, found)
    return distribution_rows(kind, mem["regret"] if kind == "iterated" else mem["weight"], nch_rows(choices), **hyper)

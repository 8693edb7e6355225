"""A naive restatement of the abstraction atlas (include/rp_mi355x.h "abstraction atlas"): the reference's derived tables
(daybook/src/schema.rs:78-173, lloyd/src/lookup.rs:86-119) and explorer queries (portal/src/topology/api.rs) over one street's
(obs, abs) table.  Python ints for the BIGINT order, ``sorted`` per bucket, explicit ``np.float32`` folds one operation at a time,
neighbours ranked by (dx, abs) tuples.  Canonical suit labellings come from the CPU oracle (oracle_deuce); nothing here reads
robopoker_amd."""
from __future__ import annotations

import math

import numpy as np

import oracle_deuce as od

F = np.float32
OK, MISS, SAME, EMPTY, RANGE = 0, 1, 2, 3, 4
HIST_ABS, HIST_OBS = 0, 1
N_CARDS = (2, 5, 6, 7)
N_OBSERVATIONS = (1_326, 25_989_600, 305_377_800, 2_809_475_760)
N_ISOMORPHISMS = (169, 1_286_792, 13_960_050, 123_156_254)
N_CHILDREN = (19_600, 47, 46, 0)
SAMPLE = np.dtype([("obs", "<i8"), ("equity", "<f4"), ("density", "<f4"), ("distance", "<f4"), ("position", "<u4"), ("population", "<u4"),
                   ("abs", "<i2"), ("reserved", "u1", (2,))])
assert SAMPLE.itemsize == 32


def pair(a: int, b: int) -> int:
    """Pair::merge (lloyd/src/pair.rs:59-62)"""
    lo, hi = min(a, b), max(a, b)
    return hi * (hi - 1) // 2 + lo


def draw_index(draw: int, population: int) -> int:
    """RANDOM() * population with a caller's draw: u = (draw >> 11) * 2^-53, floor(u * population)"""
    u = float(draw >> 11) * 2.0 ** -53
    return int(math.floor(u * float(population)))


def decode(v: int):
    """From<i64> for Observation (observation.rs:144-165): (pocket, public) bit sets; a byte that is no card is dropped"""
    po = pu = 0
    if v <= 0:
        return 0, 0
    for i in range(8):
        b = v >> (8 * i)
        if b == 0:
            break
        c = (b & 0xFF) - 1
        card = 1 << c if 0 <= c < 52 else 0
        if i < 2:
            po |= card
        else:
            pu |= card
    return po, pu


def river_equity(k: int) -> np.float32:
    return F(k) / F(100.0)


def transition_rows(counts, weight):
    """a centroid's rows as rp_artifact_write_transitions writes them: (bin, dx) for the bins with a count, dx descending, stable"""
    rows = [(b, F(int(c)) / F(int(weight))) for b, c in enumerate(counts) if c]
    return sorted(rows, key=lambda r: -float(r[1]))


def get_equity(rows, next_equity):
    """schema.rs:100-107 in f32: (fold of dx * next.equity, fold of dx, their quotient or 0)"""
    num, den = F(0.0), F(0.0)
    for b, dx in rows:
        num = F(num + F(dx * next_equity[b]))
        den = F(den + dx)
    return num, den, (F(0.0) if not rows or den == 0 else F(num / den))


class Atlas:
    def __init__(self, street, obs, abs_, K, future=None, weight=None, tri=None, row_equity=None, nxt=None):
        self.street, self.K, self.n = street, K, len(obs)
        self.obs = [int(o) for o in obs]
        self.abs = [int(a) for a in abs_]
        self.row = {o: i for i, o in enumerate(self.obs)}
        self.tri, self.row_equity, self.future, self.weight = tri, row_equity, future, weight
        self.bins = 0 if future is None else future.shape[1]
        buckets = [[] for _ in range(K)]
        for i, a in enumerate(self.abs):
            buckets[a].append(i)
        self.bucket = [sorted(rows, key=lambda i: self.obs[i]) for rows in buckets]  # rows of bucket k by obs ascending
        self.population = np.array([len(b) for b in self.bucket], np.uint32)
        self.offset = np.concatenate([[0], np.cumsum(self.population)]).astype(np.uint32)
        self.members = np.array([i for b in self.bucket for i in b], np.uint32)
        self.position = np.zeros(self.n, np.uint32)
        for b in self.bucket:
            for p, i in enumerate(b):
                self.position[i] = p
        if street == 3:
            self.rows = None
            self.equity = np.array([river_equity(k) for k in range(K)], F)
        else:
            self.rows = [transition_rows(future[k], weight[k]) for k in range(K)]
            folds = [get_equity(r, nxt.equity) for r in self.rows]
            self.fold = np.array([f[0] for f in folds], F)
            self.equity = np.array([f[2] for f in folds], F)

    # ---- helpers
    def find(self, obs: int) -> int:
        po, pu = decode(int(obs))
        if bin(po).count("1") != 2 or bin(pu).count("1") + 2 != N_CARDS[self.street] or po & pu:
            return -1
        return self.row.get(od.obs_i64(*od.isomorphism(po, pu)), -1)

    def distance1(self, a: int, b: int) -> np.float32:
        return F(0.0) if a == b else F(self.tri[pair(a, b)])

    def _member(self, k: int, i: int, population: int):
        s = np.zeros((), SAMPLE)
        s["abs"], s["equity"], s["population"] = self.street << 8 | k, self.equity[k], population
        s["density"] = F(population) / F(N_ISOMORPHISMS[self.street])
        if population:
            s["position"], s["obs"] = i, self.obs[self.bucket[k][i]]
        return s

    # ---- queries
    def describe(self, obs, wrt=None):
        out, status = np.zeros(len(obs), SAMPLE), np.zeros(len(obs), np.uint8)
        for q, o in enumerate(obs):
            row = self.find(o)
            if row < 0:
                status[q] = MISS
            elif wrt is not None and wrt[q] >= self.K:
                status[q] = RANGE
            else:
                k = self.abs[row]
                s = out[q]
                s["obs"], s["abs"], s["equity"], s["population"], s["position"] = self.obs[row], self.street << 8 | k, self.equity[k], \
                    self.population[k], self.position[row]
                s["density"] = F(self.population[k]) / F(N_OBSERVATIONS[self.street])
                if wrt is not None:
                    if wrt[q] == k:
                        status[q] = SAME
                    else:
                        s["distance"] = self.tri[pair(k, int(wrt[q]))]
        return out, status

    def obs_equity(self, obs):
        out, status = np.zeros(len(obs), F), np.zeros(len(obs), np.uint8)
        for q, o in enumerate(obs):
            row = self.find(o)
            if row < 0:
                status[q] = MISS
            elif self.street == 3:
                out[q] = self.row_equity[row]
            elif not self.rows[self.abs[row]]:
                status[q] = EMPTY
            else:
                out[q] = self.fold[self.abs[row]]
        return out, status

    def pick(self, abs_, draw):
        out, status = np.zeros(len(abs_), SAMPLE), np.zeros(len(abs_), np.uint8)
        for q, (k, d) in enumerate(zip(abs_, draw)):
            k = int(k)
            if k >= self.K:
                status[q] = RANGE
                continue
            pop = int(self.population[k])
            out[q] = self._member(k, draw_index(int(d), pop) if pop else 0, pop)
            status[q] = OK if pop else EMPTY
        return out, status

    def neighbors(self, wrt, k, farthest=False, draws=None):
        out, status = np.zeros((len(wrt), k), SAMPLE), np.zeros((len(wrt), k), np.uint8)
        for q, w in enumerate(wrt):
            w = int(w)
            if w >= self.K:
                status[q] = RANGE
                continue
            ranked = sorted(((-float(self.tri[pair(c, w)]) if farthest else float(self.tri[pair(c, w)]), c) for c in range(self.K) if c != w))
            for j, (_, c) in enumerate(ranked[:k]):
                pop = int(self.population[c])
                s = self._member(c, draw_index(int(draws[q][j]), pop) if draws is not None and pop else 0, pop if draws is not None else 0)
                s["population"], s["density"], s["distance"] = pop, F(pop) / F(N_ISOMORPHISMS[self.street]), self.tri[pair(c, w)]
                out[q, j] = s
                status[q, j] = EMPTY if draws is not None and not pop else OK
        return out, status

    def distance(self, a, b):
        return np.array([F(np.nan) if x >= self.K or y >= self.K else self.distance1(int(x), int(y)) for x, y in zip(a, b)], F)

    def histograms(self, kind, ids):
        counts, status = np.zeros((len(ids), self.bins), np.uint32), np.zeros(len(ids), np.uint8)
        for q, i in enumerate(ids):
            if kind == HIST_ABS:
                k = int(i)
                if k >= self.K:
                    status[q] = RANGE
                    continue
            else:
                row = self.find(i)
                if row < 0:
                    status[q] = MISS
                    continue
                k = self.abs[row]
            if not self.rows[k]:
                status[q] = EMPTY
            for b, dx in self.rows[k]:
                if kind == HIST_ABS:
                    counts[q, b] = int(F(dx * F(1000.0)))  # truncated (api.rs:207)
                else:
                    counts[q, b] = math.floor(float(F(dx * F(N_CHILDREN[self.street]))) + 0.5)  # roundf, half away from zero
        return counts, status

    def window(self, abs_, start, count):
        out, got = np.zeros((len(abs_), count), np.int64), np.zeros(len(abs_), np.uint8)
        for q, (k, s) in enumerate(zip(abs_, start)):
            rows = self.bucket[int(k)][int(s):int(s) + count] if k < self.K else []
            out[q, :len(rows)] = [self.obs[i] for i in rows]
            got[q] = len(rows)
        return out, got

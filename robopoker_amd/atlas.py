"""The abstraction atlas (include/rp_mi355x.h, "abstraction atlas"): the reference's derived tables — ``abstraction.population`` /
``equity`` (daybook/src/schema.rs:78-173), ``isomorphism.position`` (lloyd/src/lookup.rs:86-119) — and the batched queries of its
``TopologyAPI`` (portal/src/topology/api.rs) over one street's lookup, metric and transitions.  The tables are derived and the queries
answered on the device (robopoker_amd/csrc/atlas.hip, atlas.hpp); there is no CPU path.  Randomness is the caller's: every ``draw`` is
a uint64, u = (draw >> 11) * 2^-53.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch  # imported BEFORE the first HIP call of librp_mi355x.so: one HIP runtime per process

from . import _lib
from .deuce import STREETS, _street

SAMPLE_DTYPE = np.dtype([("obs", "<i8"), ("equity", "<f4"), ("density", "<f4"), ("distance", "<f4"), ("position", "<u4"),
                         ("population", "<u4"), ("abs", "<i2"), ("reserved", "u1", (2,))])  # rp_atlas_sample
N_NEIGHBORS = 6  # the explorer's default k (api.rs)
MAX_NEIGHBORS = 16
MAX_WINDOW = 16


def _ptr(a):
    return None if a is None else a.ctypes.data


class Atlas:
    """rp_atlas over one street.  ``obs`` / ``abstraction``: the street's lookup as device tensors (pretraining.Artifacts);
    ``future`` / ``future_weight`` / ``metric``: the layer's centroids and distances (host arrays); ``below``: the Atlas of the next
    street; ``row_equity``: the river's equities (device f32 tensor)."""

    def __init__(self, street, obs: torch.Tensor, abstraction: torch.Tensor, K: int | None = None, future=None, future_weight=None,
                 metric=None, row_equity: torch.Tensor | None = None, below: "Atlas | None" = None):
        assert obs.dtype == torch.int64 and abstraction.dtype == torch.uint8 and obs.is_cuda and abstraction.is_cuda
        assert obs.numel() == abstraction.numel()
        self._lib = _lib.load()
        self.street, self.n, self.device = _street(street), obs.numel(), obs.device
        if K is None:
            K = future.shape[0] if future is not None else int(abstraction.max().item()) + 1
        self.K = int(K)
        fc = None if future is None else np.ascontiguousarray(future, np.uint32)
        fw = None if future_weight is None else np.ascontiguousarray(future_weight, np.uint64)
        tri = None if metric is None else np.ascontiguousarray(metric, np.float32)
        self.bins = 0 if fc is None else int(fc.shape[1])
        self.has_metric = tri is not None and self.K > 1
        self.metric = tri
        if row_equity is not None:
            assert row_equity.dtype == torch.float32 and row_equity.is_cuda and row_equity.numel() == self.n
            row_equity = row_equity.contiguous()
        self.below = below
        self._obs, self._abstraction, self._row_equity = obs.contiguous(), abstraction.contiguous(), row_equity
        torch.cuda.synchronize(self.device)
        h = C.c_void_p()
        _lib.check(self._lib.rp_atlas_create(self.device.index or 0, self.street, self.n, self._obs.data_ptr(),
                                             self._abstraction.data_ptr(), self.K, _ptr(fc), _ptr(fw), self.bins, _ptr(tri),
                                             None if row_equity is None else row_equity.data_ptr(), below._h if below is not None else None,
                                             C.byref(h)))
        self._h = h

    @classmethod
    def chain(cls, arts: dict) -> dict:
        """river -> turn -> flop -> preflop from ``pretraining.run``'s artifacts (whichever of the four streets are present, the
        river first); the river's equity column is left out (pass ``row_equity`` to the constructor to have it)."""
        out, below = {}, None
        for name in ("rive", "turn", "flop", "pref"):
            a = arts.get(name)
            if a is None:
                continue
            if name == "rive":
                below = cls(name, a.obs, a.abstraction, K=101)
            else:
                below = cls(name, a.obs, a.abstraction, future=a.future, future_weight=a.future_weight, metric=a.metric, below=below)
            out[name] = below
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rp_atlas_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    # ---- the derived tables
    def tables(self) -> dict:
        """population[K], offset[K + 1], equity[K], position[n], members[n] as numpy arrays"""
        t = {"population": np.zeros(self.K, np.uint32), "offset": np.zeros(self.K + 1, np.uint32), "equity": np.zeros(self.K, np.float32),
             "position": np.zeros(self.n, np.uint32), "members": np.zeros(self.n, np.uint32)}
        _lib.check(self._lib.rp_atlas_tables(self._h, *(t[f].ctypes.data for f in ("population", "offset", "equity", "position", "members"))))
        return t

    def tables_device(self) -> dict:
        dev = self.device
        t = {"population": torch.zeros(self.K, dtype=torch.int32, device=dev), "offset": torch.zeros(self.K + 1, dtype=torch.int32, device=dev),
             "equity": torch.zeros(self.K, dtype=torch.float32, device=dev), "position": torch.zeros(self.n, dtype=torch.int32, device=dev),
             "members": torch.zeros(self.n, dtype=torch.int32, device=dev)}
        torch.cuda.synchronize(dev)
        _lib.check(self._lib.rp_atlas_tables(self._h, *(t[f].data_ptr() for f in ("population", "offset", "equity", "position", "members"))))
        return t

    def create_ms(self) -> tuple[float, float]:
        """device time of the create: (the (abs, obs) sort, everything else)"""
        a, b = C.c_double(), C.c_double()
        _lib.check(self._lib.rp_atlas_create_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # ---- host forms: numpy in, numpy out
    def describe(self, obs, wrt=None):
        o = np.ascontiguousarray(obs, np.int64)
        w = None if wrt is None else np.ascontiguousarray(wrt, np.uint8)
        out, status = np.zeros(o.size, SAMPLE_DTYPE), np.zeros(o.size, np.uint8)
        _lib.check(self._lib.rp_atlas_describe(self._h, o.size, o.ctypes.data, _ptr(w), out.ctypes.data, status.ctypes.data))
        return out, status

    def obs_equity(self, obs):
        o = np.ascontiguousarray(obs, np.int64)
        out, status = np.zeros(o.size, np.float32), np.zeros(o.size, np.uint8)
        _lib.check(self._lib.rp_atlas_obs_equity(self._h, o.size, o.ctypes.data, out.ctypes.data, status.ctypes.data))
        return out, status

    def pick(self, abstraction, draw):
        a, d = np.ascontiguousarray(abstraction, np.uint8), np.ascontiguousarray(draw, np.uint64)
        assert a.size == d.size
        out, status = np.zeros(a.size, SAMPLE_DTYPE), np.zeros(a.size, np.uint8)
        _lib.check(self._lib.rp_atlas_pick(self._h, a.size, a.ctypes.data, d.ctypes.data, out.ctypes.data, status.ctypes.data))
        return out, status

    def neighbors(self, wrt, k: int = N_NEIGHBORS, farthest: bool = False, draws=None):
        w = np.ascontiguousarray(wrt, np.uint8)
        d = None if draws is None else np.ascontiguousarray(draws, np.uint64)
        assert d is None or d.shape == (w.size, k)
        out, status = np.zeros((w.size, k), SAMPLE_DTYPE), np.zeros((w.size, k), np.uint8)
        _lib.check(self._lib.rp_atlas_neighbors(self._h, w.size, w.ctypes.data, k, int(farthest), _ptr(d), out.ctypes.data, status.ctypes.data))
        return out, status

    def distance(self, a, b):
        a, b = np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8)
        assert a.size == b.size
        out = np.zeros(a.size, np.float32)
        _lib.check(self._lib.rp_atlas_distance(self._h, a.size, a.ctypes.data, b.ctypes.data, out.ctypes.data))
        return out

    def histograms(self, kind: str, ids):
        i = np.ascontiguousarray(ids, np.int64 if kind == "obs" else np.uint8)
        counts, status = np.zeros((i.size, self.bins), np.uint32), np.zeros(i.size, np.uint8)
        _lib.check(self._lib.rp_atlas_histograms(self._h, i.size, _lib.ATLAS_HIST[kind], i.ctypes.data, counts.ctypes.data, status.ctypes.data))
        return counts, status

    def members(self, abstraction, start, count: int):
        a, s = np.ascontiguousarray(abstraction, np.uint8), np.ascontiguousarray(start, np.uint32)
        assert a.size == s.size
        out, got = np.zeros((a.size, count), np.int64), np.zeros(a.size, np.uint8)
        _lib.check(self._lib.rp_atlas_members(self._h, a.size, a.ctypes.data, s.ctypes.data, count, out.ctypes.data, got.ctypes.data))
        return out, got

    # ---- obs_distance / obs_abs_distance (api.rs:138-154): two histograms under the NEXT street's metric, minimize().cost()
    def _cost(self, hx: torch.Tensor, hy: torch.Tensor, hp=None) -> np.ndarray:
        from .lloyd import default_sinkhorn
        if self.below is None or self.below.metric is None:
            raise ValueError("the reference has no metric over the river's bins (lloyd/src/metric.rs:101): no observation distance on the turn")
        out = torch.zeros(hx.shape[0], dtype=torch.float32, device=self.device)
        hp = hp or default_sinkhorn()
        torch.cuda.synchronize(self.device)
        if hx.shape[0]:
            _lib.check(self._lib.rp_sinkhorn_cost_device(self.bins, hx.shape[0], hx.data_ptr(), hy.data_ptr(), self.below.metric.ctypes.data,
                                                         C.byref(hp), self.device.index or 0, out.data_ptr(), None))
        return out.cpu().numpy()

    def obs_distance(self, obs1, obs2, hp=None):
        """(cost[n], status[n]): status is the larger of the two observations' histogram statuses; a cost is meaningful where it is 0"""
        a, b = (torch.from_numpy(np.ascontiguousarray(o, np.int64)).to(self.device) for o in (obs1, obs2))
        (hx, sx), (hy, sy) = self.histograms_device("obs", a), self.histograms_device("obs", b)
        return self._cost(hx, hy, hp), torch.maximum(sx, sy).cpu().numpy()

    def obs_abs_distance(self, obs, abstraction, hp=None):
        a = torch.from_numpy(np.ascontiguousarray(obs, np.int64)).to(self.device)
        b = torch.from_numpy(np.ascontiguousarray(abstraction, np.uint8)).to(self.device)
        (hx, sx), (hy, sy) = self.histograms_device("obs", a), self.histograms_device("abs", b)
        return self._cost(hx, hy, hp), torch.maximum(sx, sy).cpu().numpy()

    def save(self, directory: str) -> dict:
        """writes ``abstraction.<street>`` and ``isomorphism.<street>`` (rp_artifact_write_abstraction / _isomorphism) from the handle's
        tables and the lookup it was made of (the constructor's tensors, kept by reference); returns the two paths"""
        import os
        name = next(k for k, v in STREETS.items() if v == self.street)
        t = self.tables()
        paths = {"abstraction": os.path.join(directory, f"abstraction.{name}"), "isomorphism": os.path.join(directory, f"isomorphism.{name}")}
        _lib.check(self._lib.rp_artifact_write_abstraction(paths["abstraction"].encode(), self.street, self.K, t["population"].ctypes.data,
                                                           t["equity"].ctypes.data))
        o, a = self._obs.cpu().numpy(), self._abstraction.cpu().numpy()
        e = None if self._row_equity is None else self._row_equity.cpu().numpy()
        _lib.check(self._lib.rp_artifact_write_isomorphism(paths["isomorphism"].encode(), self.street, self.n, o.ctypes.data, a.ctypes.data,
                                                           _ptr(e), t["position"].ctypes.data))
        return paths

    # ---- device forms: torch tensors on the atlas' device in and out (records as uint8 [n][32]: view with SAMPLE_DTYPE on the host)
    def _dev(self, t: torch.Tensor, dtype) -> torch.Tensor:
        assert t.dtype == dtype and t.is_cuda
        return t.contiguous()

    def describe_device(self, obs: torch.Tensor, wrt: torch.Tensor | None = None):
        o = self._dev(obs, torch.int64)
        w = None if wrt is None else self._dev(wrt, torch.uint8)
        out = torch.zeros((o.numel(), 32), dtype=torch.uint8, device=self.device)
        status = torch.zeros(o.numel(), dtype=torch.uint8, device=self.device)
        torch.cuda.synchronize(self.device)
        _lib.check(self._lib.rp_atlas_describe_device(self._h, o.numel(), o.data_ptr(), None if w is None else w.data_ptr(), out.data_ptr(),
                                                      status.data_ptr()))
        return out, status

    def obs_equity_device(self, obs: torch.Tensor):
        o = self._dev(obs, torch.int64)
        out = torch.zeros(o.numel(), dtype=torch.float32, device=self.device)
        status = torch.zeros(o.numel(), dtype=torch.uint8, device=self.device)
        torch.cuda.synchronize(self.device)
        _lib.check(self._lib.rp_atlas_obs_equity_device(self._h, o.numel(), o.data_ptr(), out.data_ptr(), status.data_ptr()))
        return out, status

    def pick_device(self, abstraction: torch.Tensor, draw: torch.Tensor):
        """``draw``: int64 tensor holding the uint64 bit patterns"""
        a, d = self._dev(abstraction, torch.uint8), self._dev(draw, torch.int64)
        out = torch.zeros((a.numel(), 32), dtype=torch.uint8, device=self.device)
        status = torch.zeros(a.numel(), dtype=torch.uint8, device=self.device)
        torch.cuda.synchronize(self.device)
        _lib.check(self._lib.rp_atlas_pick_device(self._h, a.numel(), a.data_ptr(), d.data_ptr(), out.data_ptr(), status.data_ptr()))
        return out, status

    def neighbors_device(self, wrt: torch.Tensor, k: int = N_NEIGHBORS, farthest: bool = False, draws: torch.Tensor | None = None):
        w = self._dev(wrt, torch.uint8)
        d = None if draws is None else self._dev(draws, torch.int64)
        out = torch.zeros((w.numel(), k, 32), dtype=torch.uint8, device=self.device)
        status = torch.zeros((w.numel(), k), dtype=torch.uint8, device=self.device)
        torch.cuda.synchronize(self.device)
        _lib.check(self._lib.rp_atlas_neighbors_device(self._h, w.numel(), w.data_ptr(), k, int(farthest), None if d is None else d.data_ptr(),
                                                       out.data_ptr(), status.data_ptr()))
        return out, status

    def distance_device(self, a: torch.Tensor, b: torch.Tensor):
        a, b = self._dev(a, torch.uint8), self._dev(b, torch.uint8)
        out = torch.zeros(a.numel(), dtype=torch.float32, device=self.device)
        torch.cuda.synchronize(self.device)
        _lib.check(self._lib.rp_atlas_distance_device(self._h, a.numel(), a.data_ptr(), b.data_ptr(), out.data_ptr()))
        return out

    def histograms_device(self, kind: str, ids: torch.Tensor):
        i = self._dev(ids, torch.int64 if kind == "obs" else torch.uint8)
        counts = torch.zeros((i.numel(), self.bins), dtype=torch.int32, device=self.device)
        status = torch.zeros(i.numel(), dtype=torch.uint8, device=self.device)
        torch.cuda.synchronize(self.device)
        _lib.check(self._lib.rp_atlas_histograms_device(self._h, i.numel(), _lib.ATLAS_HIST[kind], i.data_ptr(), counts.data_ptr(), status.data_ptr()))
        return counts, status

    def members_device(self, abstraction: torch.Tensor, start: torch.Tensor, count: int):
        a, s = self._dev(abstraction, torch.uint8), self._dev(start, torch.int32)
        out = torch.zeros((a.numel(), count), dtype=torch.int64, device=self.device)
        got = torch.zeros(a.numel(), dtype=torch.uint8, device=self.device)
        torch.cuda.synchronize(self.device)
        _lib.check(self._lib.rp_atlas_members_device(self._h, a.numel(), a.data_ptr(), s.data_ptr(), count, out.data_ptr(), got.data_ptr()))
        return out, got


__all__ = ["Atlas", "SAMPLE_DTYPE", "N_NEIGHBORS", "STREETS"]

"""CPU-side checks of the abstraction atlas ABI (include/rp_mi355x.h, rp_atlas_*): the symbols exist, the record has the size the header
states and the offsets of its mirrors, every argument check that needs no device answers before one is asked for, and the two artifact
writers round-trip through rp_pgcopy_read, SQL NULL included."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

from robopoker_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rp_mi355x.h")
QUERIES = ("rp_atlas_describe", "rp_atlas_obs_equity", "rp_atlas_pick", "rp_atlas_neighbors", "rp_atlas_distance", "rp_atlas_histograms",
           "rp_atlas_members")
CALLS = ("rp_atlas_create", "rp_atlas_destroy", "rp_atlas_shape", "rp_atlas_tables", "rp_atlas_create_ms", "rp_sinkhorn_cost_device",
         "rp_artifact_write_abstraction", "rp_artifact_write_isomorphism") + QUERIES + tuple(q + "_device" for q in QUERIES)
INVALID, UNSUPPORTED = _lib.RP_ERR_INVALID, _lib.RP_ERR_UNSUPPORTED


def test_symbols_exist():
    lib, text = _lib.load(), open(HEADER).read()
    for name in CALLS:
        assert re.search(r"RP_API\s+int\s+" + name + r"\s*\(", text) and hasattr(lib, name) and name in _lib.declared_symbols(), name


def test_record_size_and_offsets(tmp_path):
    import atlas_model as AM
    from robopoker_amd import atlas
    text = open(HEADER).read()
    assert re.search(r"\}\s*rp_atlas_sample;\s*/\*\s*32 bytes\s*\*/", text) and C.sizeof(_lib.AtlasSample) == 32 == atlas.SAMPLE_DTYPE.itemsize
    offsets = {f: getattr(_lib.AtlasSample, f).offset for f, _ in _lib.AtlasSample._fields_}
    assert offsets == {f: atlas.SAMPLE_DTYPE.fields[f][1] for f in atlas.SAMPLE_DTYPE.names} == {f: AM.SAMPLE.fields[f][1] for f in AM.SAMPLE.names}
    for name, value in _lib.ATLAS_STATUS.items():
        assert re.search(r"RP_ATLAS_%s = %d\b" % (name.upper(), value), text) and getattr(AM, name.upper()) == value
    assert re.search(r"RP_ATLAS_HIST_ABS = 0, RP_ATLAS_HIST_OBS = 1", text) and _lib.ATLAS_HIST == {"abs": 0, "obs": 1}
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    if cc is not None:
        src = tmp_path / "sizes.c"
        src.write_text('#include <stddef.h>\n#include "rp_mi355x.h"\n_Static_assert(sizeof(rp_atlas_sample) == 32, "size");\n' +
                       "".join(f'_Static_assert(offsetof(rp_atlas_sample, {f}) == {o}, "{f}");\n' for f, o in offsets.items()))
        subprocess.check_call([cc, "-std=c11", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)])


def test_create_checks_its_arguments_before_it_needs_a_device():
    lib = _lib.load()
    h = C.c_void_p()
    p = C.c_void_p(64)  # never dereferenced: every call below is refused first
    out = C.byref(h)

    def create(street=3, n=8, obs=p, abs_=p, K=101, fc=None, fw=None, bins=0, tri=None, eq=None, nxt=None, out=out):
        return lib.rp_atlas_create(0, street, n, obs, abs_, K, fc, fw, bins, tri, eq, nxt, out)

    assert create(out=None) == create(obs=None) == create(abs_=None) == create(n=0) == INVALID and b"rp_atlas_create" in lib.rp_last_error()
    assert create(street=4) == create(street=-1) == INVALID
    assert create(K=0) == create(K=257) == INVALID and b"1..256" in lib.rp_last_error()
    assert create(n=(1 << 27) + 1) == UNSUPPORTED and b"27 bits" in lib.rp_last_error()
    # the river takes no future, no metric, no next
    assert create(fc=p) == create(fw=p) == create(tri=p) == create(nxt=p) == create(bins=5) == INVALID
    # the other streets need all of future_counts, future_weight and next, and no equity column
    for street in (0, 1, 2):
        assert create(street=street, fc=p, fw=p, bins=5) == create(street=street, fc=p, nxt=p, bins=5) == create(street=street, fw=p, nxt=p, bins=5) == INVALID
    assert h.value is None


def test_queries_check_their_arguments_before_they_need_a_device():
    lib = _lib.load()
    p = C.c_void_p(64)
    for form in ("", "_device"):
        f = lambda name: getattr(lib, name + form)  # noqa: E731
        assert f("rp_atlas_describe")(None, 1, p, None, p, p) == INVALID and b"rp_atlas_describe" in lib.rp_last_error()
        assert f("rp_atlas_obs_equity")(None, 1, p, p, p) == INVALID
        assert f("rp_atlas_pick")(None, 1, p, p, p, p) == INVALID
        assert f("rp_atlas_neighbors")(None, 1, p, 6, 0, None, p, p) == INVALID
        assert f("rp_atlas_distance")(None, 1, p, p, p) == INVALID
        assert f("rp_atlas_histograms")(None, 1, 0, p, p, p) == INVALID
        assert f("rp_atlas_members")(None, 1, p, p, 6, p, p) == INVALID and b"rp_atlas_members" in lib.rp_last_error()
    assert lib.rp_atlas_shape(None, None, None, None, None) == lib.rp_atlas_tables(None, None, None, None, None, None) == INVALID
    assert lib.rp_atlas_create_ms(None, None, None) == INVALID and lib.rp_atlas_destroy(None) == _lib.RP_OK
    assert lib.rp_sinkhorn_cost_device(0, 1, p, p, p, None, 0, p, None) == INVALID
    assert lib.rp_sinkhorn_cost_device(4, 1, None, p, p, None, 0, p, None) == INVALID


def read(path, types, cap):
    lib = _lib.load()
    kinds = {"h": np.int16, "i": np.int32, "q": np.int64, "f": np.float32}
    cols = [np.zeros(cap, kinds[t]) for t in types]
    ptrs = (C.c_void_p * len(types))(*(c.ctypes.data for c in cols))
    n = C.c_uint64()
    _lib.check(lib.rp_pgcopy_read(str(path).encode(), types.encode(), cap, ptrs, C.byref(n)))
    return n.value, cols


def test_the_two_artifact_files_round_trip(tmp_path):
    lib = _lib.load()
    rng = np.random.default_rng(0)
    K, n = 5, 40
    population, equity = rng.integers(0, 1 << 27, K).astype(np.uint32), rng.random(K).astype(np.float32)
    path = tmp_path / "abstraction"
    _lib.check(lib.rp_artifact_write_abstraction(str(path).encode(), 2, K, population.ctypes.data, equity.ctypes.data))
    rows, (a, s, p, e) = read(path, "hhif", 8)
    assert rows == K and a[:K].tolist() == [2 << 8 | k for k in range(K)] and (s[:K] == 2).all()
    assert np.array_equal(p[:K], population.astype(np.int32)) and e[:K].tobytes() == equity.tobytes()
    assert path.stat().st_size == 19 + K * (2 + 4 * 4 + 2 + 2 + 4 + 4) + 2
    obs = rng.integers(1, 1 << 56, n).astype(np.int64)
    labels, position, eq = rng.integers(0, 256, n).astype(np.uint8), rng.integers(0, 1 << 27, n).astype(np.uint32), rng.random(n).astype(np.float32)
    for column in (eq, None):
        path = tmp_path / ("isomorphism" + ("" if column is None else ".eq"))
        _lib.check(lib.rp_artifact_write_isomorphism(str(path).encode(), 3, n, obs.ctypes.data, labels.ctypes.data,
                                                     None if column is None else column.ctypes.data, position.ctypes.data))
        rows, (o, a, e, p) = read(path, "qhfi", n)
        assert rows == n and np.array_equal(o, obs) and np.array_equal(a, (3 << 8 | labels.astype(np.int16))) and np.array_equal(p, position.astype(np.int32))
        if column is None:  # SQL NULL: a field of length -1 and no bytes, read back as the stated NaN
            assert (e.view(np.uint32) == 0xFFFFFFFF).all() and path.stat().st_size == 19 + n * (2 + 4 * 4 + 8 + 2 + 0 + 4) + 2
            assert int(re.search(r"#define RP_PGCOPY_NULL_F32 (0x[0-9a-f]+)u", open(HEADER).read()).group(1), 16) == 0xFFFFFFFF
        else:
            assert e.tobytes() == eq.tobytes()
    # a NULL anywhere but in a float4 column is still refused
    n_rows = C.c_uint64()
    assert lib.rp_pgcopy_read(str(path).encode(), b"qhii", 0, None, C.byref(n_rows)) == INVALID
    assert lib.rp_artifact_write_abstraction(None, 2, K, population.ctypes.data, equity.ctypes.data) == INVALID
    assert lib.rp_artifact_write_abstraction(str(path).encode(), 2, 257, population.ctypes.data, equity.ctypes.data) == INVALID
    assert lib.rp_artifact_write_isomorphism(str(path).encode(), 3, n, obs.ctypes.data, labels.ctypes.data, None, None) == INVALID
    assert lib.rp_artifact_write_isomorphism(str(path).encode(), 4, n, obs.ctypes.data, labels.ctypes.data, None, position.ctypes.data) == INVALID

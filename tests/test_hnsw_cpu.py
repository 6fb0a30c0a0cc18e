"""CPU: the host side of cuvsHnsw* (cuvs_amd/csrc/hnsw_host.hpp through the C ABI, with res = 0) against the numpy twin
tests/hnsw_ref.py: ABI, search, extend, file round trip and malformed files. Integer-valued coordinates make every distance
exact and ties frequent, which is where the (distance, id) order can go wrong."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import hnsw_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

EXPORTS = ["cuvsHnswAceParamsCreate", "cuvsHnswAceParamsDestroy", "cuvsHnswIndexParamsCreate", "cuvsHnswIndexParamsDestroy",
           "cuvsHnswIndexCreate", "cuvsHnswIndexDestroy", "cuvsHnswExtendParamsCreate", "cuvsHnswExtendParamsDestroy",
           "cuvsHnswFromCagra", "cuvsHnswFromCagraWithDataset", "cuvsHnswBuild", "cuvsHnswExtend", "cuvsHnswSearchParamsCreate",
           "cuvsHnswSearchParamsDestroy", "cuvsHnswSearch", "cuvsHnswSerialize", "cuvsHnswDeserialize"]
DTYPES = [np.float32, np.float16, np.int8, np.uint8]
METRICS = {R.L2: "sqeuclidean", R.IP: "inner_product"}
HIER = {R.NONE: "none", R.CPU: "cpu", R.GPU: "gpu"}
DIMS = (5, 16, 33)


def _hnsw():
    from cuvs_amd.neighbors import hnsw

    return hnsw


def int_rows(rng, n, dim, dtype):
    """integer-valued coordinates in [-8, 8] ([0, 16] for uint8)"""
    v = rng.integers(-8, 9, size=(n, dim))
    return (v + 8).astype(dtype) if np.dtype(dtype) == np.uint8 else v.astype(dtype)


def twin_index(rows, metric, hierarchy, degree=8, ef_construction=40):
    ix = R.Index.from_graph(rows, R.exact_knn_graph(rows, degree, metric), metric, hierarchy, ef_construction)
    if hierarchy == R.CPU:
        ix.build_cpu_hierarchy()
    elif hierarchy == R.GPU:
        ix.build_exact_hierarchy()
    return ix


# ---------------------------------------------------------------- ABI
def test_abi_layout_matches_the_reference_header(tmp_path):
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(GOLD, "hnsw_abi_probe.c"), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode() == open(os.path.join(GOLD, "hnsw_abi_layout.txt")).read()


def test_exports_config_and_defaults(tmp_path):
    from cuvs_amd._lib import lib

    L = lib()
    assert len(EXPORTS) == 17 and all(hasattr(L, s) for s in EXPORTS)
    src = tmp_path / "c.c"
    src.write_text("#include <cuvs/core/all.h>\n#ifndef CUVS_BUILD_CAGRA_HNSWLIB\n#error no hnsw\n#endif\n"
                   "int main(void) { struct cuvsHnswSearchParams p = {0, 0}; return p.ef + (int)NONE + (int)CPU - (int)GPU + 1; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    h = _hnsw()
    p = h.IndexParams()
    assert (p.hierarchy, p.ef_construction, p.num_threads, p.M, p.metric, p.ace_params) == ("gpu", 200, 0, 32, "sqeuclidean", None)
    assert not p._p.contents.ace_params
    a = C.POINTER(h._CAceParams)()
    assert L.cuvsHnswAceParamsCreate(C.byref(a)) == 1
    assert (a.contents.npartitions, a.contents.build_dir, a.contents.use_disk, a.contents.max_host_memory_gb,
            a.contents.max_gpu_memory_gb) == (0, b"/tmp/hnsw_ace_build", False, 0.0, 0.0)
    assert L.cuvsHnswAceParamsDestroy(a) == 1
    s = h.SearchParams()
    assert (s.ef, s.num_threads) == (200, 0)
    assert h.ExtendParams().num_threads == 0
    i = h.Index()
    assert i._p.contents.addr == 0


# ---------------------------------------------------------------- search
CASES = [(di, mi, hi) for di in range(4) for mi in range(2) for hi in range(3)]


@pytest.mark.parametrize("di,mi,hi", CASES)
def test_search_equals_the_twin(tmp_path, di, mi, hi):
    h = _hnsw()
    dtype, metric, hierarchy = DTYPES[di], (R.L2, R.IP)[mi], (R.NONE, R.CPU, R.GPU)[hi]
    dim = DIMS[(di + mi + hi) % 3]
    rng = np.random.default_rng(100 * di + 10 * mi + hi)
    rows = int_rows(rng, 600, dim, dtype)
    queries = int_rows(rng, 24, dim, dtype)
    ix = twin_index(rows, metric, hierarchy)
    if hierarchy != R.NONE:
        assert ix.maxlevel >= 2
    blob = ix.to_bytes()
    f = tmp_path / "twin.bin"
    f.write_bytes(blob)
    got = h.load(h.IndexParams(hierarchy=HIER[hierarchy]), f, dim, dtype, METRICS[metric])
    want_i, want_d = ix.search(queries, 10, 32)
    d1, i1 = h.search(h.SearchParams(ef=32, num_threads=1), got, queries, 10)
    d4, i4 = h.search(h.SearchParams(ef=32, num_threads=4), got, queries, 10)
    assert np.array_equal(i1, want_i) and np.array_equal(d1, want_d)
    assert np.array_equal(i4, want_i) and np.array_equal(d4, want_d)
    # ef below k: the search runs with k
    want_i, want_d = ix.search(queries[:6], 10, 3)
    d, i = h.search(h.SearchParams(ef=3, num_threads=2), got, queries[:6], 10)
    assert np.array_equal(i, want_i) and np.array_equal(d, want_d)
    # round trip
    out = tmp_path / "back.bin"
    h.save(out, got)
    assert out.read_bytes() == blob
    # the twin's own reader
    back = R.Index.from_bytes(blob, dim, dtype, metric, hierarchy)
    assert back.to_bytes() == blob


@pytest.mark.parametrize("hierarchy", [R.NONE, R.GPU])
def test_k_beyond_the_reachable_rows_is_padded(tmp_path, hierarchy):
    h = _hnsw()
    rng = np.random.default_rng(5)
    rows = int_rows(rng, 600, 16, np.float32)
    graph = np.zeros((600, 8), dtype=np.uint32)  # islands of 20 rows: a walk never leaves the one it starts in
    for i in range(600):
        b = i // 20 * 20
        graph[i] = [b + (i - b + j + 1) % 20 for j in range(8)]
    ix = R.Index.from_graph(rows, graph, R.L2, hierarchy)
    if hierarchy == R.GPU:
        ix.build_exact_hierarchy()
    f = tmp_path / "islands.bin"
    f.write_bytes(ix.to_bytes())
    got = h.load(h.IndexParams(hierarchy=HIER[hierarchy]), f, 16, np.float32)
    queries = int_rows(rng, 8, 16, np.float32)
    want_i, want_d = ix.search(queries, 30, 64)
    d, i = h.search(h.SearchParams(ef=64, num_threads=2), got, queries, 30)
    assert np.array_equal(i, want_i) and np.array_equal(d, want_d)
    assert (i[:, 20:] == np.iinfo(np.uint64).max).all() and (d[:, 20:] == np.finfo(np.float32).max).all()
    assert (i[:, :20] < 600).all()


# ---------------------------------------------------------------- extend
@pytest.mark.parametrize("dtype,metric,dim", [(np.float32, R.L2, 16), (np.int8, R.IP, 5), (np.float16, R.L2, 33)])
def test_extend_writes_the_twins_bytes(tmp_path, dtype, metric, dim):
    h = _hnsw()
    rng = np.random.default_rng(11)
    rows = int_rows(rng, 560, dim, dtype)
    ix = twin_index(rows[:500], metric, R.CPU)
    f = tmp_path / "base.bin"
    f.write_bytes(ix.to_bytes())
    got = h.load(h.IndexParams(hierarchy="cpu"), f, dim, dtype, METRICS[metric])
    h.extend(h.ExtendParams(num_threads=3), got, rows[500:])
    out = tmp_path / "extended.bin"
    h.save(out, got)
    ix.extend(rows[500:])
    assert ix.n == 560 and out.read_bytes() == ix.to_bytes()
    queries = int_rows(rng, 8, dim, dtype)
    want_i, want_d = ix.search(queries, 10, 40)
    d, i = h.search(h.SearchParams(ef=40, num_threads=2), got, queries, 10)
    assert np.array_equal(i, want_i) and np.array_equal(d, want_d)
    assert (i >= 500).any()


def test_extend_refuses_a_base_layer_only_index_and_foreign_rows(tmp_path):
    from cuvs_amd._lib import CuvsError

    h = _hnsw()
    rows = int_rows(np.random.default_rng(3), 100, 5, np.uint8)
    f = tmp_path / "none.bin"
    f.write_bytes(twin_index(rows, R.L2, R.NONE).to_bytes())
    got = h.load(h.IndexParams(hierarchy="none"), f, 5, np.uint8)
    with pytest.raises(CuvsError, match="immutable"):
        h.extend(h.ExtendParams(), got, rows[:3])
    with pytest.raises(CuvsError, match="type mismatch between index and queries"):
        h.search(h.SearchParams(), got, rows[:3].astype(np.int8), 3)
    with pytest.raises(CuvsError, match="neighbors should be of type uint64_t"):
        h.search(h.SearchParams(), got, rows[:3], 3, neighbors=np.zeros((3, 3), dtype=np.int64))
    with pytest.raises(CuvsError, match="distances should be of type float32"):
        h.search(h.SearchParams(), got, rows[:3], 3, distances=np.zeros((3, 3), dtype=np.float64))
    with pytest.raises(CuvsError, match="Unsupported metric type was used"):
        h.load(h.IndexParams(hierarchy="none"), f, 5, np.uint8, "cosine")
    with pytest.raises(CuvsError, match="not built"):
        h.search(h.SearchParams(), h.Index(), rows[:3], 3)


# ---------------------------------------------------------------- malformed files
def test_malformed_files_are_refused_with_text(tmp_path):
    from cuvs_amd._lib import CuvsError

    h = _hnsw()
    rows = int_rows(np.random.default_rng(9), 200, 5, np.int8)
    ix = twin_index(rows, R.L2, R.GPU)
    blob = ix.to_bytes()
    per = 4 * ix.maxM0 + 4 + 5 + 8
    up = 96 + 200 * per
    first = int(np.nonzero(ix.levels >= 1)[0][0])  # the first row with an upper block
    flat = int(np.nonzero(ix.levels == 0)[0][0])
    pos = up + 4 * first + sum(u.size * 4 for u in ix.upper[:first])
    assert struct.unpack_from("<I", blob, pos)[0] == ix.levels[first] * (4 * ix.maxM + 4)

    def patched(off, fmt, *v):
        b = bytearray(blob)
        struct.pack_into(fmt, b, off, *v)
        return bytes(b)

    cases = {
        "too short": blob[:-1],
        "too long": blob + b"\0",
        "header only": blob[:96],
        "half a header": blob[:40],
        "empty": b"",
        "record size": patched(24, "<Q", per + 1),
        "label offset": patched(32, "<Q", per - 7),
        "offset data": patched(40, "<Q", 4 * ix.maxM0),
        "maxM0": patched(64, "<Q", ix.maxM0 + 1),
        "link id": patched(96 + 4, "<I", 200),
        "count above cap": patched(96, "<I", ix.maxM0 + 1),
        "entry": patched(52, "<i", 200),
        "negative entry": patched(52, "<i", -1),
        "top level": patched(48, "<i", 33),
        "negative top level": patched(48, "<i", -1),
        "row level above the top": patched(48, "<i", 0),
        "row count": patched(16, "<Q", 2 ** 40),
        "no rows": patched(16, "<Q", 0),
        "rows above max": patched(8, "<Q", 100),
        "upper bytes": patched(pos, "<I", 4 * ix.maxM + 8),
        "upper count above cap": patched(pos + 4, "<I", ix.maxM + 1),
        "upper link id": patched(pos + 8, "<I", 4000),
        "upper link below its level": patched(pos + 8, "<I", flat),
        "entry below the top level": patched(52, "<i", flat),
    }
    assert ix.upper[first][0, 0] >= 1
    for name, b in cases.items():
        f = tmp_path / "bad.bin"
        f.write_bytes(b)
        with pytest.raises(CuvsError) as e:
            h.load(h.IndexParams(hierarchy="gpu"), f, 5, np.int8)
        assert len(str(e.value)) > 10, name
    f = tmp_path / "ok.bin"
    f.write_bytes(blob)
    for dim, dtype in ((6, np.int8), (5, np.float32), (5, np.float16)):
        with pytest.raises(CuvsError, match="does not fit"):
            h.load(h.IndexParams(hierarchy="gpu"), f, dim, dtype)
    with pytest.raises(CuvsError, match="Cannot open"):
        h.load(h.IndexParams(hierarchy="gpu"), tmp_path / "missing.bin", 5, np.int8)
    h.load(h.IndexParams(hierarchy="gpu"), f, 5, np.int8)
    h.load(h.IndexParams(hierarchy="gpu"), f, 5, np.uint8)  # same record size: the caller's word is taken


# ---------------------------------------------------------------- sanitizers
def test_host_code_under_the_sanitizers(tmp_path):
    exe = tmp_path / "hnsw_host_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-pthread", "-I",
                           os.path.join(ROOT, "cuvs_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "hnsw_host_test.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "hnsw host OK" in out.stdout

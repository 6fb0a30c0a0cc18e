"""CPU: the Vamana C ABI (include/cuvs/neighbors/vamana.h) has the reference's layout and defaults and refuses bad arguments
before it touches a device; the file writers of tests/vamana_ref.py produce hand-computed bytes; the graphs that the numpy
restatement builds pass the reference's own graph checks and its recall floor."""
import ctypes as C
import functools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import vamana_ref as ref
from cuvs_amd._lib import CuvsError, Tensor, lib
from cuvs_amd.neighbors import vamana

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_every_prototype_is_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cuvs", "neighbors", "vamana.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"CUVS_EXPORT\s+cuvsError_t\s+(cuvsVamana\w+)\s*\(", text)))
    assert names == ["cuvsVamanaBuild", "cuvsVamanaIndexCreate", "cuvsVamanaIndexDestroy", "cuvsVamanaIndexGetDims",
                     "cuvsVamanaIndexParamsCreate", "cuvsVamanaIndexParamsDestroy", "cuvsVamanaSerialize"]
    for n in names + ["cuvsAmdVamanaIndexGetGraph", "cuvsAmdVamanaIndexGetMedoid", "cuvsAmdVamanaGreedySearch",
                      "cuvsAmdVamanaRobustPrune", "cuvsAmdVamanaSerializeSectorAligned"]:
        assert hasattr(lib(), n), n


def test_struct_layout_matches_the_reference_header(tmp_path):
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(GOLDEN, "vamana_abi_probe.c"), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode() == open(os.path.join(GOLDEN, "vamana_abi_layout.txt")).read()
    assert C.sizeof(vamana._CParams) == 36 and C.sizeof(vamana._CIndex) == 16


def test_parameter_defaults():
    p = C.POINTER(vamana._CParams)()
    assert lib().cuvsVamanaIndexParamsCreate(C.byref(p)) == 1
    c = p.contents
    assert (c.metric, c.graph_degree, c.visited_size, c.vamana_iters, c.queue_size, c.reverse_batchsize) == (0, 32, 64, 1.0, 127,
                                                                                                             1000000)
    assert (c.alpha, c.max_fraction, c.batch_base) == (np.float32(1.2), np.float32(0.06), 2.0)
    assert lib().cuvsVamanaIndexParamsDestroy(p) == 1
    assert lib().cuvsVamanaIndexParamsCreate(None) == 0
    q = vamana.IndexParams()
    assert (q.metric, q.graph_degree, q.visited_size, q.vamana_iters, q.queue_size, q.reverse_batchsize) == (
        "sqeuclidean", 32, 64, 1.0, 127, 1000000)
    q = vamana.IndexParams(graph_degree=64, visited_size=128, vamana_iters=1.5, alpha=1.0, max_fraction=1.0, batch_base=3.0,
                           queue_size=15, reverse_batchsize=100)
    assert (q.graph_degree, q.visited_size, q.vamana_iters, q.alpha, q.max_fraction, q.batch_base, q.queue_size,
            q.reverse_batchsize) == (64, 128, 1.5, 1.0, 1.0, 3.0, 15, 100)


def _build_error(params, data):
    idx = vamana.Index()
    lib().cuvsSetLastErrorText(b"")
    assert lib().cuvsVamanaBuild(C.c_size_t(0), params._p, Tensor(data).ptr, idx._p) == 0
    return lib().cuvsGetLastErrorText().decode()


def test_refusals_come_before_the_device_is_touched():
    x = np.zeros((20, 8), dtype=np.float32)
    # well-formed arguments reach the null handle: validation itself lets them through
    assert "null cuvsResources_t" in _build_error(vamana.IndexParams(), x)
    for dt in (np.int8, np.uint8):
        assert "null cuvsResources_t" in _build_error(vamana.IndexParams(), x.astype(dt))
    assert "Currently only L2Expanded metric is supported" in _build_error(vamana.IndexParams(metric="inner_product"), x)
    for degree in (0, 16, 33, 48, 512):
        assert "Provided graph_degree not currently supported" in _build_error(
            vamana.IndexParams(graph_degree=degree, visited_size=1024), x)
    for degree in (32, 64, 128, 256):
        assert "null cuvsResources_t" in _build_error(vamana.IndexParams(graph_degree=degree, visited_size=2 * degree), x)
    assert "visited_size must be > graph_degree" in _build_error(vamana.IndexParams(graph_degree=64, visited_size=64), x)
    assert "visited_size must be > graph_degree" in _build_error(vamana.IndexParams(graph_degree=32, visited_size=8), x)
    assert "vamana_iters must be at least 1.0 to insert the entire input dataset" in _build_error(
        vamana.IndexParams(vamana_iters=0.5), x)
    assert "Unsupported dataset DLtensor dtype: 2 and bits: 64" in _build_error(vamana.IndexParams(), x.astype(np.float64))
    assert "Unsupported dataset DLtensor dtype: 2 and bits: 16" in _build_error(vamana.IndexParams(), x.astype(np.float16))
    assert "Unsupported dataset DLtensor dtype: 0 and bits: 32" in _build_error(vamana.IndexParams(), x.astype(np.int32))
    # limits of this implementation
    assert "visited_size above 1024" in _build_error(vamana.IndexParams(visited_size=2048), x)
    assert "row-major" in _build_error(vamana.IndexParams(), np.zeros((20, 16), dtype=np.float32)[:, ::2])


def test_an_index_that_is_not_built_is_refused():
    idx = vamana.Index()
    d = C.c_int(0)
    assert lib().cuvsVamanaIndexGetDims(idx._p, C.byref(d)) == 0
    assert "not built" in lib().cuvsGetLastErrorText().decode()
    assert lib().cuvsVamanaSerialize(C.c_size_t(0), b"/nonexistent/x", idx._p, C.c_bool(True)) == 0
    m = C.c_uint32(0)
    assert lib().cuvsAmdVamanaIndexGetMedoid(idx._p, C.byref(m)) == 0
    assert not idx.trained
    with pytest.raises(CuvsError, match="not built"):
        idx.graph


def test_parameters_that_no_build_can_use_are_refused():
    x = np.zeros((20, 8), dtype=np.float32)
    for alpha in (0.99, 0.0, -1.0, float("nan")):  # no pass of the prune would run: every pruned node would lose its edges
        assert "alpha must be at least 1.0" in _build_error(vamana.IndexParams(alpha=alpha), x)
    assert "null cuvsResources_t" in _build_error(vamana.IndexParams(alpha=1.0), x)
    for f in (float("nan"), -0.5):
        assert "max_fraction must not be negative" in _build_error(vamana.IndexParams(max_fraction=f), x)
    for f in (0.0, 1e30, float("inf")):  # clamped to one row and to all rows
        assert "null cuvsResources_t" in _build_error(vamana.IndexParams(max_fraction=f), x)
    for b in (float("nan"), 0.5):
        assert "batch_base must be at least 1.0" in _build_error(vamana.IndexParams(batch_base=b), x)
    assert "null cuvsResources_t" in _build_error(vamana.IndexParams(batch_base=1e30), x)
    # a batch whose edges a 32-bit index cannot number: 2^23 rows of degree 256 in one batch
    big = np.zeros((1 << 23, 1), dtype=np.uint8)
    assert "2^31 edges or more" in _build_error(vamana.IndexParams(graph_degree=256, visited_size=512, max_fraction=1.0), big)
    assert "null cuvsResources_t" in _build_error(vamana.IndexParams(graph_degree=256, visited_size=512, max_fraction=0.5), big)


def test_cpp_surface_instantiates(tmp_path):
    """cuvs::neighbors::vamana of include/cuvs_amd/neighbors.hpp: build<T> for the three row types and serialize compile as C++17."""
    src = tmp_path / "v.cpp"
    src.write_text(
        "#include <cuvs_amd/neighbors.hpp>\n"
        "#include <cstdint>\n"
        "namespace v = cuvs::neighbors::vamana;\n"
        "template <typename T> int use(const cuvs::resources& res, cuvs::device_matrix_view<const T> rows) {\n"
        "  v::index_params p;\n"
        "  p.graph_degree = 64; p.visited_size = 128;\n"
        "  v::index<T> idx = v::build<T>(res, p, rows);\n"
        "  v::serialize(res, \"prefix\", idx);\n"
        "  v::serialize(res, \"prefix\", idx, false, true);\n"
        "  return idx.dim() + (int)idx.medoid();\n"
        "}\n"
        "template int use<float>(const cuvs::resources&, cuvs::device_matrix_view<const float>);\n"
        "template int use<int8_t>(const cuvs::resources&, cuvs::device_matrix_view<const int8_t>);\n"
        "template int use<uint8_t>(const cuvs::resources&, cuvs::device_matrix_view<const uint8_t>);\n"
        "int main() { v::index_params p; return p.graph_degree == 32 && p.queue_size == 127 ? 0 : 1; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_rounding_of_visited_size_and_the_batch_schedule():
    assert ref.Params(visited_size=100).visited == 128 and ref.Params(graph_degree=64, visited_size=65).visited == 128
    assert ref.Params(visited_size=64).visited == 64
    p = ref.Params()
    assert p.max_batch(10) == 1 and p.max_batch(33) == 1 and p.max_batch(1000) == 60  # int(0.06 n), at least one row
    assert ref.Params(max_fraction=3.0).max_batch(10) == 10
    sizes = [m for _, m in ref.batches(1000, p)]
    assert sizes[:7] == [1, 2, 4, 8, 16, 32, 60] and sum(sizes) == 1000 and max(sizes) == 60
    b = ref.batches(300, ref.Params(vamana_iters=1.5, max_fraction=1.0))
    assert sum(m for _, m in b) == 450 and b[-1] == (0, 150)
    for n in (1, 2, 10, 1000):
        assert sorted(ref.insert_order(n).tolist()) == list(range(n))
    assert ref.insert_order(1000).tolist() != list(range(1000))


# ---- file layouts against hand-computed bytes: 3 nodes, degree 4, medoid 2
_G = np.array([[1, 2, 0xFFFFFFFF, 0xFFFFFFFF], [0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF], [0, 1, 0xFFFFFFFF, 0xFFFFFFFF]],
              dtype=np.uint32)


def test_index_file_bytes():
    want = struct.pack("<QIIQ", 24 + 4 * (3 + 2 + 3), 2, 2, 0)
    want += struct.pack("<III", 2, 1, 2) + struct.pack("<II", 1, 0) + struct.pack("<III", 2, 0, 1)
    got = ref.index_bytes(_G, 2)
    assert got == want and struct.unpack("<Q", got[:8])[0] == len(got) == 56


def test_data_file_bytes():
    x = np.array([[1, -2], [3, 4], [5, 6]], dtype=np.int8)
    assert ref.data_bytes(x) == struct.pack("<ii", 3, 2) + bytes([1, 254, 3, 4, 5, 6])
    xf = np.array([[1.5, 2.0]], dtype=np.float32)
    assert ref.data_bytes(xf) == struct.pack("<ii", 1, 2) + struct.pack("<ff", 1.5, 2.0)


def test_sector_aligned_bytes_packed_nodes():
    x = np.array([[1, 2], [3, 4], [5, 6]], dtype=np.uint8)
    got = ref.disk_index_bytes(_G, 2, x)
    node_len = (2 + 1) * 4 + 2  # 14 bytes: 292 nodes per sector
    assert len(got) == 2 * 4096
    assert got[:80] == struct.pack("<ii9Q", 9, 1, 3, 2, 2, node_len, 4096 // node_len, 0, 0, 0, 2 * 4096)
    assert got[80:4096] == bytes(4096 - 80)
    nodes = (bytes([1, 2]) + struct.pack("<III", 2, 1, 2) + bytes([3, 4]) + struct.pack("<III", 1, 0, 0)
             + bytes([5, 6]) + struct.pack("<III", 2, 0, 1))
    assert got[4096:4096 + 42] == nodes and got[4096 + 42:] == bytes(4096 - 42)


def test_sector_aligned_bytes_node_spanning_sectors():
    x = np.arange(3 * 1100, dtype=np.float32).reshape(3, 1100)  # 4400-byte rows: a node takes two sectors
    got = ref.disk_index_bytes(_G, 2, x)
    node_len = 12 + 4400
    assert len(got) == (1 + 3 * 2) * 4096
    assert got[:80] == struct.pack("<ii9Q", 9, 1, 3, 1100, 2, node_len, 0, 0, 0, 0, 7 * 4096)
    for i, edges in enumerate(([2, 1, 2], [1, 0], [2, 0, 1])):
        at = 4096 * (1 + 2 * i)
        node = x[i].tobytes() + struct.pack(f"<{len(edges)}I", *edges)
        assert got[at:at + len(node)] == node
        assert got[at + len(node):at + 8192] == bytes(8192 - len(node))


# ---- the twin's own graphs: the reference's CheckGraph conditions (ann_vamana.cuh:71-109) and recall floor (:301)
@functools.lru_cache(maxsize=None)
def twin_graph(dim):
    rng = np.random.default_rng(1234)
    x = rng.normal(0.1, 2.0, (1000, dim)).astype(np.float32)
    g, med = ref.build(x, ref.Params())
    return x, g, med


@pytest.mark.parametrize("dim", [1, 3, 64, 137])
def test_twin_graph_passes_the_reference_graph_checks(dim):
    x, g, med = twin_graph(dim)
    max_degree, fraction = ref.check_graph(g, 1000, dim, 32)
    print(f"dim {dim}: max degree {max_degree}, edge fraction {fraction:.3f}, medoid {med}")
    assert max_degree >= min(32, dim)
    assert fraction > 0.75
    assert med == int(np.argmin(((x.astype(np.float64) - x.astype(np.float64).mean(axis=0)) ** 2).sum(axis=1)))


@pytest.mark.parametrize("dim", [1, 3, 64, 137])
def test_twin_graph_recall(dim):
    x, g, med = twin_graph(dim)
    q = np.random.default_rng(4321).normal(0.1, 2.0, (100, dim)).astype(np.float32)
    d = ((q.astype(np.float64)[:, None, :] - x.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    truth = np.argsort(d, axis=1, kind="stable")[:, :10]
    r = ref.recall(ref.beam_search(x, g, med, q, 10), truth)
    print(f"dim {dim}: recall@10 {r:.4f}")
    assert r >= 0.2

"""CPU: IVF-RaBitQ's C entry points (exported symbols, parameter defaults) and the numpy restatement tests/ivf_rabitq_ref.py on
its own: bit-stream round trips, the file, the scaling factor against the library's host code, and the recall of the contract
against exact kNN with the reference's floors (tests/golden/ivf_rabitq_reference_table.json)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import ivf_rabitq_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cuvs_amd", "libcuvs_c.so")
TABLE = json.load(open(os.path.join(ROOT, "tests", "golden", "ivf_rabitq_reference_table.json")))
FLOORS = TABLE["floors"]


def test_symbols_exported_and_parameter_defaults():
    from cuvs_amd.neighbors import ivf_rabitq

    lib = C.CDLL(LIB)
    for s in ("Build", "Search", "Serialize", "Deserialize", "Export", "ExportCenters", "ScalingFactor", "LastSearchStats",
              "IndexGetNLists", "IndexGetDim", "IndexGetSize", "IndexGetBitsPerDim", "IndexCreate", "IndexDestroy"):
        assert hasattr(lib, "cuvsAmdIvfRabitq" + s), s
    p = C.POINTER(ivf_rabitq._CIndexParams)()
    assert lib.cuvsAmdIvfRabitqIndexParamsCreate(C.byref(p)) == 1
    v = p.contents
    # cpp/include/cuvs/neighbors/ivf_rabitq.hpp: index_params
    assert (v.metric, v.n_lists, v.bits_per_dim, v.kmeans_n_iters, v.max_train_points_per_cluster, v.fast_quantize_flag,
            v.streaming_batch_size, v.force_streaming) == (0, 1024, 3, 20, 256, True, 100000, False)
    assert lib.cuvsAmdIvfRabitqIndexParamsDestroy(p) == 1
    sp = C.POINTER(ivf_rabitq._CSearchParams)()
    assert lib.cuvsAmdIvfRabitqSearchParamsCreate(C.byref(sp)) == 1
    assert (sp.contents.n_probes, sp.contents.mode) == (20, 2)  # QUANT4
    assert lib.cuvsAmdIvfRabitqSearchParamsDestroy(sp) == 1
    assert ivf_rabitq.SEARCH_MODES == {"lut16": 0, "lut32": 1, "quant4": 2, "quant8": 3}
    idx = C.POINTER(ivf_rabitq._CIndex)()
    assert lib.cuvsAmdIvfRabitqIndexCreate(C.byref(idx)) == 1
    n = C.c_int64(0)
    assert lib.cuvsAmdIvfRabitqIndexGetNLists(idx, C.byref(n)) == 0  # not built: CUVS_ERROR
    assert lib.cuvsAmdIvfRabitqIndexDestroy(idx) == 1


def test_header_is_valid_c99_and_cxx17(tmp_path):
    import subprocess

    src = tmp_path / "h.c"
    src.write_text("#include <cuvs_amd/ivf_rabitq.h>\n#include <cuvs_amd/ivf_rabitq.h>\n"
                   "int main(void) { cuvsAmdIvfRabitqIndex_t i = 0; (void)i; return CUVS_AMD_IVF_RABITQ_QUANT4 == 2 ? 0 : 1; }\n")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", inc, str(src)])
    subprocess.check_call(["g++", "-std=c++17", "-Werror", "-fsyntax-only", "-x", "c++", "-I", inc, str(src)])


@pytest.mark.parametrize("ex", range(0, 9))
def test_code_streams_round_trip(ex):
    rng = np.random.default_rng(ex)
    D, n = 192, 37
    bits = rng.integers(0, 2, (n, D), dtype=np.uint8)
    words = R.pack_bits(bits)
    assert words.shape == (n, D // 32) and words.dtype == np.uint32
    assert np.array_equal(R.unpack_bits(words, D), bits)
    # dimension 32 w + i at bit 31 - i
    one = np.zeros((1, D), np.uint8)
    one[0, 32 + 3] = 1
    assert R.pack_bits(one)[0].tolist() == [0, 1 << 28, 0, 0, 0, 0]
    codes = rng.integers(0, 1 << ex, (n, D), dtype=np.uint8) if ex else np.zeros((n, D), np.uint8)
    stream = R.pack_ex(codes, ex)
    assert stream.shape == (n, D * ex // 8)
    assert np.array_equal(R.unpack_ex(stream, D, ex), codes)
    if ex == 3:  # MSB first: codes 5, 1, 7 -> 101 001 11|1...
        c = np.zeros((1, 64), np.uint8)
        c[0, :3] = (5, 1, 7)
        assert R.pack_ex(c, 3)[0, :2].tolist() == [0b10100111, 0b10000000]


def test_lane_sum_order():
    # 1 + 2^-24 twice in one lane rounds away; spread over two lanes it survives the butterfly
    t = np.zeros(128, np.float32)
    t[0], t[64] = 1.0, 2.0 ** -24
    assert R.lane_sum(t) == np.float32(1.0)
    t[64], t[32] = 0.0, 2.0 ** -23
    assert R.lane_sum(t) == np.float32(1.0 + 2.0 ** -23)


@pytest.mark.parametrize("D,ex", [(64, 1), (64, 2), (128, 4), (256, 8)])
def test_scaling_factor_matches_the_library(D, ex):
    from cuvs_amd.neighbors import ivf_rabitq

    t = R.scaling_factor(D, ex)
    assert t.dtype == np.float32 and t > 0
    assert np.float32(ivf_rabitq.scaling_factor(D, ex)).view(np.uint32) == t.view(np.uint32)


def _rotation(D, seed=3):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((D, D)))
    return q.astype(np.float32)


def _lloyd(x, n_lists, iters=5, seed=1):
    rng = np.random.default_rng(seed)
    c = x[rng.choice(len(x), n_lists, replace=False)].astype(np.float64)
    x64 = x.astype(np.float64)
    for _ in range(iters):
        lab = ((x64 * x64).sum(1)[:, None] - 2 * x64 @ c.T + (c * c).sum(1)[None, :]).argmin(1)
        for L in range(n_lists):
            if np.any(lab == L):
                c[L] = x64[lab == L].mean(0)
    return c.astype(np.float32)


def clustered(n, nq, seed=11):
    """64 Gaussian modes in an 8-d latent space, mapped to 64 dimensions, plus 0.05 noise"""
    rng = np.random.default_rng(seed)
    modes = rng.standard_normal((64, 8))
    lift = rng.standard_normal((8, 64)) / np.sqrt(8)

    def draw(m):
        lat = modes[rng.integers(0, 64, m)] + 0.3 * rng.standard_normal((m, 8))
        return (lat @ lift + 0.05 * rng.standard_normal((m, 64))).astype(np.float32)

    return draw(n), draw(nq)


def uniform(n, nq, seed=12):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.1, 2.0, (n, 64)).astype(np.float32), rng.uniform(0.1, 2.0, (nq, 64)).astype(np.float32))


def exact_knn(q, x, k):
    q64, x64 = q.astype(np.float64), x.astype(np.float64)
    d = (q64 * q64).sum(1)[:, None] - 2 * q64 @ x64.T + (x64 * x64).sum(1)[None, :]
    return np.argsort(d, axis=1, kind="stable")[:, :k]


def recall(found, truth):
    return sum(len(np.intersect1d(f, t)) for f, t in zip(found, truth)) / truth.size


_CACHE = {}


def _index(kind, bits):
    if (kind, bits) not in _CACHE:
        if kind not in _CACHE:
            x, q = clustered(4096, 256) if kind == "clustered" else uniform(4096, 256)
            _CACHE[kind] = (x, q, _lloyd(x, 32), exact_knn(q, x, 10))
        x, q, centers, truth = _CACHE[kind]
        _CACHE[(kind, bits)] = R.build(x, centers, _rotation(64), bits)
    return _CACHE[(kind, bits)], _CACHE[kind][1], _CACHE[kind][3]


# (bits, mode, n_probes, floor): the reference's floors - 0.5, 0.3 at one bit, 0.08 per probe up to five probes
@pytest.mark.parametrize("bits,mode,n_probes,floor", [
    (3, "quant4", 20, FLOORS["default"]), (1, "quant4", 20, FLOORS["bits_per_dim_1"]), (5, "quant8", 20, FLOORS["default"]),
    (3, "quant4", 1, 1 * FLOORS["per_probe_up_to_5_probes"]), (3, "quant4", 5, 5 * FLOORS["per_probe_up_to_5_probes"])])
def test_recall_of_the_contract_clustered(bits, mode, n_probes, floor):
    ex, q, truth = _index("clustered", bits)
    _, nb = R.search(ex, q, 10, n_probes, mode)
    r = recall(nb, truth)
    print(f"clustered bits={bits} mode={mode} n_probes={n_probes}: recall@10 {r:.3f} (floor {floor})")
    assert r >= floor


# uniform [0.1, 2.0) data, the reference's generator: only the default parameters and one probe (at 1 bit, 2 bits and 5 probes a
# correct implementation sits on the floor there)
@pytest.mark.parametrize("n_probes,floor", [(20, FLOORS["default"]), (1, FLOORS["per_probe_up_to_5_probes"])])
def test_recall_of_the_contract_uniform(n_probes, floor):
    ex, q, truth = _index("uniform", 3)
    _, nb = R.search(ex, q, 10, n_probes, "quant4")
    r = recall(nb, truth)
    print(f"uniform bits=3 n_probes={n_probes}: recall@10 {r:.3f} (floor {floor})")
    assert r >= floor


def test_screen_never_drops_a_true_head_and_modes_agree_on_the_final_distances():
    """the final distance of a candidate does not depend on the mode; only the set of survivors does"""
    ex, q, _ = _index("clustered", 3)
    d4, i4 = R.search(ex, q[:32], 10, 20, "quant4")
    d32, i32 = R.search(ex, q[:32], 10, 20, "lut32")
    both = (i4 == i32)
    assert both.mean() > 0.9
    assert np.array_equal(d4[both].view(np.uint32), d32[both].view(np.uint32))


def test_file_round_trip(tmp_path):
    ex, _, _ = _index("clustered", 3)
    p = str(tmp_path / "r.bin")
    R.write_file(p, ex, "euclidean")
    back = R.parse_file(p)
    assert (back["n"], back["dim"], back["ex_bits"], back["metric"]) == (4096, 64, 2, "euclidean")
    assert back["t"].view(np.uint32) == ex["t"].view(np.uint32)
    for name in ("list_sizes", "rotation", "centers_rot", "bit_codes", "short_factors", "ex_codes", "ex_factors", "ids"):
        assert np.array_equal(back[name], ex[name]), name
    off = R.section_offsets(4096, 64, 32, 2)
    assert off["end"] == os.path.getsize(p)
    assert off["rotation"] == 41 + 8 * 32 and off["ids"] == off["end"] - 4 * 4096

"""CPU: the C ABI and Python surface of CAGRA's VPQ compression that need no device - struct defaults, the argument
refusals of cuvsCagraBuild (made from the arguments alone, before the handle is looked at), the accessor on an unbuilt index -
and self-checks of tests/cagra_vpq_ref.py (decode and tag-3 parser on a hand-made record)."""
import ctypes as C

import numpy as np
import pytest

from tests import cagra_vpq_ref as V


def _lib():
    from cuvs_amd._lib import lib

    L = lib()
    L.cuvsGetLastErrorText.restype = C.c_char_p
    return L


def test_struct_defaults_of_the_c_create():
    from cuvs_amd.neighbors.cagra import _CCompressionParams

    p = C.POINTER(_CCompressionParams)()
    assert _lib().cuvsCagraCompressionParamsCreate(C.byref(p)) == 1
    v = p.contents
    assert (v.pq_bits, v.pq_dim, v.vq_n_centers, v.kmeans_n_iters, v.vq_kmeans_trainset_fraction,
            v.pq_kmeans_trainset_fraction) == (8, 0, 0, 25, 0.0, 0.0)
    assert C.sizeof(_CCompressionParams) == 32  # tests/golden/abi_layout.txt
    assert _lib().cuvsCagraCompressionParamsDestroy(p) == 1


def test_python_params_write_their_fields_and_stay_alive():
    from cuvs_amd.neighbors import cagra

    d = cagra.CompressionParams()
    assert (d.pq_bits, d.pq_dim, d.vq_n_centers, d.kmeans_n_iters, d.vq_kmeans_trainset_fraction,
            d.pq_kmeans_trainset_fraction) == (8, 0, 0, 25, 0.0, 0.0)
    c = cagra.CompressionParams(pq_bits=8, pq_dim=16, vq_n_centers=40, kmeans_n_iters=7, vq_kmeans_trainset_fraction=0.5,
                                pq_kmeans_trainset_fraction=0.25)
    v = c._p.contents
    assert (v.pq_bits, v.pq_dim, v.vq_n_centers, v.kmeans_n_iters, v.vq_kmeans_trainset_fraction,
            v.pq_kmeans_trainset_fraction) == (8, 16, 40, 7, 0.5, 0.25)
    assert cagra.IndexParams()._p.contents.compression is None and cagra.IndexParams().compression is None
    ip = cagra.IndexParams(compression=c)
    assert ip.compression is c  # the C struct points into c: the params keep it alive
    assert ip._p.contents.compression == C.cast(c._p, C.c_void_p).value


REFUSALS = [
    # metric, compression kwargs, (n, dim), part of the message
    ("inner_product", {}, (300, 8), "VPQ compression is only supported with L2Expanded"),
    ("euclidean", {}, (300, 8), "VPQ compression is only supported with L2Expanded"),
    ("sqeuclidean", {"pq_bits": 4}, (300, 8), "pq_bits = 8 only"),
    ("sqeuclidean", {"pq_dim": 4}, (300, 10), "multiple of pq_dim"),
    ("sqeuclidean", {"pq_dim": 2}, (300, 16), "pq_len = dim / pq_dim of 2 or 4 only"),
    ("sqeuclidean", {"pq_dim": 8}, (300, 8), "pq_len = dim / pq_dim of 2 or 4 only"),
    ("sqeuclidean", {}, (255, 8), "at least 256 rows"),
    ("sqeuclidean", {"pq_kmeans_trainset_fraction": 0.5}, (300, 8), "PQ training set"),
    ("sqeuclidean", {"vq_n_centers": 301}, (300, 8), "vq_n_centers (301) exceeds the number of rows"),
]


@pytest.mark.parametrize("metric,kw,shape,text", REFUSALS, ids=[r[3][:24].replace(" ", "_") + str(i) for i, r in enumerate(REFUSALS)])
def test_build_refuses_from_the_arguments_alone(metric, kw, shape, text):
    """no handle is given (0): the refusal must come before the handle or the device is touched"""
    from cuvs_amd._lib import Tensor
    from cuvs_amd.neighbors import cagra

    ip = cagra.IndexParams(metric=metric, graph_degree=16, intermediate_graph_degree=32, compression=cagra.CompressionParams(**kw))
    t = Tensor(np.zeros(shape, np.float32))
    idx = cagra.Index()
    assert _lib().cuvsCagraBuild(C.c_size_t(0), ip._p, t.ptr, idx._p) == 0
    assert text in _lib().cuvsGetLastErrorText().decode()
    assert idx._p.contents.addr == 0


def test_vpq_info_on_an_unbuilt_index():
    from cuvs_amd.neighbors import cagra

    idx = cagra.Index()
    out = (C.c_uint32 * 5)()
    assert _lib().cuvsAmdCagraIndexGetVpqInfo(idx._p, out) == 0
    assert "not built" in _lib().cuvsGetLastErrorText().decode()
    assert not idx.compressed
    for s in ("cuvsAmdCagraIndexGetVpq", "cuvsAmdCagraIndexGetVpqInfo"):
        assert hasattr(_lib(), s)


def test_decode_and_parser_agree_on_a_hand_made_record(tmp_path):
    # dim 6, pq_len 2: pq_dim 3, so a row is 4 label bytes + 3 codes + 1 padding byte
    vq = np.array([[1, 2, 3, 4, 5, 6], [10, 20, 30, 40, 50, 60]], np.float16)
    pq = np.zeros((256, 2), np.float16)
    pq[:, 0] = np.arange(256) / 4.0
    pq[:, 1] = -np.arange(256) / 8.0
    codes = np.array([[1, 0, 0, 0, 4, 0, 255, 0], [0, 0, 0, 0, 1, 2, 3, 0]], np.uint8)
    assert V.row_len(3) == 8 and V.row_len(4) == 8 and V.row_len(5) == 12 and V.row_len(192) == 196
    labels, c, pad = V.split_codes(codes, 3)
    assert labels.tolist() == [1, 0] and c.tolist() == [[4, 0, 255], [1, 2, 3]] and not pad.any()
    assert np.array_equal(V.join_codes(labels, c), codes)
    x = V.decode(vq, pq, codes)
    want = np.array([[10 + 1.0, 20 - 0.5, 30 + 0.0, 40 - 0.0, 50 + 63.75, 60 - 31.875],
                     [1 + 0.25, 2 - 0.125, 3 + 0.5, 4 - 0.25, 5 + 0.75, 6 - 0.375]], np.float32)
    assert x.dtype == np.float32 and np.array_equal(x, want)
    graph = np.array([[1], [0]], np.uint32)
    path = str(tmp_path / "hand.cagra")
    V.write_cagra_vpq(path, graph, vq, pq, codes, dtype=np.float16)
    f = V.parse_cagra_vpq(path)
    assert (f["prefix"], f["version"], f["size"], f["dim"], f["graph_degree"], f["metric"]) == (b"<e2\0", 5, 2, 6, 1, 0)
    assert (f["tag"], f["cuda_dtype"], f["n_rows"], f["ds_dim"], f["vq_n_centers"], f["pq_n_centers"], f["pq_len"],
            f["encoded_row_length"]) == (3, V.CUDA_R_16F, 2, 6, 2, 256, 2, 8)
    assert np.array_equal(f["graph"], graph)
    assert f["vq_code_book"].dtype == np.float16 and np.array_equal(f["vq_code_book"], vq) and np.array_equal(f["pq_code_book"], pq)
    assert np.array_equal(V.decode(f["vq_code_book"], f["pq_code_book"], f["data"]), want)

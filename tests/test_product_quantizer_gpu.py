"""GPU: the product quantizer (cuvsProductQuantizer*, cuvs_amd.preprocessing.quantize.pq). The encoder is pinned on supplied
codebooks (cuvsAmdProductQuantizerFromCodebooks) against an fp64 bound and against the plain encoder in a child process; the
training is checked with the reference's own C++ and Python tests and against a numpy Lloyd baseline."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from cuvs_amd._lib import CuvsError
from cuvs_amd.common import Resources
from cuvs_amd.neighbors import brute_force
from cuvs_amd.preprocessing.quantize import pq
from tests import product_quantizer_ref as P
from tests.pq_encode_worker import all_cases, counters, encode_case, num_cus

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_IDS = ["n%d-pqdim%d-len%d-bits%d-sub%d-vq%d" % c for c in P.ENCODER_CASES]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------- 1, 3, 4: encoder and decoder
@pytest.mark.parametrize("case", P.ENCODER_CASES, ids=CASE_IDS)
def test_encoder_exactness_packing_and_decoding(case):
    n, pq_dim, pq_len, bits, subspaces, vq = case
    before = counters()
    q, x, book, vq_book, packed, labels = encode_case(case)
    after = counters()
    # the path the fallback rule names really ran
    assert tuple(a - b for a, b in zip(after, before)) == ((1, 0, 0) if P.uses_default_path(pq_len) else (0, 1, 0))
    assert (q.pq_bits, q.pq_dim, q.encoded_dim, q.use_vq) == (bits, pq_dim, P.encoded_dim(pq_dim, bits), vq)
    assert np.array_equal(q.pq_codebook.cpu().numpy(), book)
    assert tuple(q.vq_codebook.shape) == (vq_book.shape if vq else (0, 0))
    assert packed.shape == (n, P.encoded_dim(pq_dim, bits)) and P.unused_bits_are_zero(packed, pq_dim, bits)
    codes = P.unpack_codes(packed, pq_dim, bits)
    assert codes.max() < (1 << bits)
    if vq:
        # 4: the bound of the expanded form kmeans_predict evaluates
        assert labels.max() < len(vq_book)
        x64, v64 = x.astype(np.float64), vq_book.astype(np.float64)
        d = ((x64[:, None, :] - v64[None, :, :]) ** 2).sum(2)
        slack = 8 * (x.shape[1] + 4) * 2.0 ** -24 * ((x64 ** 2).sum(1) + (v64 ** 2).sum(1).max())
        assert (d[np.arange(n), labels] <= d.min(1) + slack).all()
    # 1: every (row, subspace): d64(code) <= d64(best) (1 + 4 (pq_len + 2) 2^-24)
    r = P.residual(x, vq_book, labels)
    worst, differ = P.distance_excess(r, book, codes, pq_dim, pq_len, bits, subspaces)
    allowed = 4 * (pq_len + 2) * 2.0 ** -24
    print(f"{case}: {differ} of {n * pq_dim} codes differ from the fp64 argmin, worst excess {worst:.3e}, allowed {allowed:.3e}")
    assert worst <= allowed
    # 3: InverseTransform is book[code] (+ vq[label]) exactly
    lab_t = None if labels is None else dev(labels.astype(np.uint32))
    out = pq.inverse_transform(q, dev(packed), vq_labels=lab_t)
    want = P.decode(book, codes, pq_len, bits, subspaces, vq_book, labels)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("pq_len,bits", [(8, 8), (3, 5), (64, 6)])
def test_exact_duplicates_get_the_lowest_index(pq_len, bits):
    rng = np.random.default_rng(11)
    book_n, pq_dim, n = 1 << bits, 5, 700
    book = rng.normal(0, 1, (pq_dim * book_n, pq_len)).astype(np.float32)
    dup = {}
    for j in range(pq_dim):  # entry `a` of every subspace is repeated at three later places
        a = int(rng.integers(0, book_n // 2))
        others = rng.choice(np.arange(a + 1, book_n), 3, replace=False)
        book[j * book_n + others] = book[j * book_n + a]
        dup[j] = (a, others)
    x = np.concatenate([book[j * book_n + dup[j][0]][None, :].repeat(n, 0) for j in range(pq_dim)], axis=1)
    x = (x + np.float32(1e-3) * rng.normal(0, 1, x.shape)).astype(np.float32)
    params = pq.QuantizerParams(pq_bits=bits, pq_dim=pq_dim)
    q = pq.from_codebooks(params, dev(book))
    packed, _ = pq.transform(q, dev(x))
    codes = P.unpack_codes(packed.cpu().numpy(), pq_dim, bits)
    for j in range(pq_dim):
        assert (codes[:, j] == dup[j][0]).all(), j


# ---------------------------------------------------------------------------------------------- 2: default == plain
def test_default_path_equals_plain_path(tmp_path):
    out = str(tmp_path / "plain.npz")
    env = dict(os.environ, CUVS_AMD_DEBUG_SWITCHES="1", CUVS_AMD_PQ_ENCODE="plain")
    subprocess.run([sys.executable, "-m", "tests.pq_encode_worker", out], cwd=ROOT, env=env, check=True, timeout=600)
    plain = np.load(out)
    cases = all_cases()
    assert tuple(plain["counters"]) == (0, len(cases), 0)  # the child ran the plain encoder for every case
    before = counters()
    for i, case in enumerate(cases):
        _, _, _, _, codes, labels = encode_case(case)
        assert np.array_equal(codes, plain[f"codes{i}"]), case
        if labels is not None:
            assert np.array_equal(labels, plain[f"labels{i}"]), case
    after = counters()
    n_default = sum(P.uses_default_path(c[2]) for c in cases)
    n_multi = sum(P.runs_multi_row(c, num_cus()) for c in cases)
    assert n_multi >= len(P.MULTI_ROW_SHAPES)
    assert tuple(a - b for a, b in zip(after, before)) == (n_default, len(cases) - n_default, n_multi)


@pytest.mark.parametrize("shape", range(len(P.MULTI_ROW_SHAPES)), ids=["pqdim%d-len%d-bits%d-sub%d-vq%d" % c for c in P.MULTI_ROW_SHAPES])
def test_multi_row_encoder(shape):
    """pq_encode_kernel<PL, R> with R = 4 (PL 1, 2, 4, 8) and R = 2 (PL 16, 32): the row count is just past the launcher's
    threshold for this device, the tail a multiple of neither 256 nor 256 R. The launch counter shows that R > 1 ran; the fp64
    bound of the exactness test holds on the rows at the start, around the row-group and workgroup boundaries and in the tail;
    the bytes of ALL rows are compared with the plain encoder in test_default_path_equals_plain_path."""
    case = P.multi_row_cases(num_cus())[shape]
    n, pq_dim, pq_len, bits, subspaces, vq = case
    before = counters()
    q, x, book, vq_book, packed, labels = encode_case(case)
    after = counters()
    assert tuple(a - b for a, b in zip(after, before)) == (1, 0, 1)
    assert packed.shape == (n, P.encoded_dim(pq_dim, bits)) and P.unused_bits_are_zero(packed, pq_dim, bits)
    rows = P.boundary_rows(n, pq_len)
    codes = P.unpack_codes(packed[rows], pq_dim, bits)
    r = P.residual(x[rows], vq_book, None if labels is None else labels[rows])
    worst, differ = P.distance_excess(r, book, codes, pq_dim, pq_len, bits, subspaces)
    allowed = 4 * (pq_len + 2) * 2.0 ** -24
    print(f"{case}: {differ} of {len(rows) * pq_dim} sampled codes differ from the fp64 argmin, worst excess {worst:.3e}, allowed {allowed:.3e}")
    assert worst <= allowed
    lab_t = None if labels is None else dev(labels[rows].astype(np.uint32))
    out = pq.inverse_transform(q, dev(packed[rows]), vq_labels=lab_t)
    want = P.decode(book, codes, pq_len, bits, subspaces, vq_book, None if labels is None else labels[rows])
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------- 5: the reference's C++ table
KM, KMB = "kmeans", "kmeans_balanced"
# product_quantization.cu:317-427: n_samples, n_features, pq_bits, pq_dim, kmeans type, n_vq_centers, use_subspaces, use_vq, host
CPP_TABLE = [
    (1, 64, 4, 8, KMB, 0, True, False, False), (512, 1, 8, 1, KMB, 0, True, True, False),
    (4096, 1024, 10, 4, KMB, 0, False, False, False), (20, 2, 4, 1, KMB, 0, False, True, False),
    (200, 8, 7, 2, KM, 2, False, True, False), (299, 3000, 8, 64, KMB, 0, False, True, False),
    (100, 64, 4, 8, KMB, 0, False, False, False), (100, 90, 6, 10, KMB, 0, False, False, True),
    (300, 128, 7, 32, KMB, 0, True, True, True), (500, 40, 5, 8, KM, 0, False, False, False),
    (500, 60, 6, 6, KMB, 4, True, True, True), (500, 128, 5, 8, KM, 0, True, False, False),
    (1000, 320, 8, 64, KM, 0, True, True, False), (1000, 384, 8, 64, KMB, 0, True, True, False),
    (1000, 40, 4, 10, KMB, 0, False, False, False), (3000, 1024, 4, 32, KM, 0, False, False, False),
    (1000, 2048, 4, 128, KMB, 0, True, True, False), (50000, 1024, 8, 128, KMB, 0, False, True, False),
    (50000, 2048, 8, 128, KMB, 10, True, True, True),
]


@pytest.mark.parametrize("row", CPP_TABLE, ids=["-".join(str(v) for v in r) for r in CPP_TABLE])
def test_reference_cpp_table(row):
    """Every row of the reference's `inputs<float>` with the reference's own bound. Measured on an MI355X: all rows pass; the
    closest is (200, 8, 7 bits, pq_dim 2, classic k-means, 2 VQ centres, one shared book): worst row error 0.859 against 1.141."""
    n, dim, bits, pq_dim, ktype, n_vq, subspaces, vq, host = row
    x = P.make_blobs(n, dim, 42)
    params = pq.QuantizerParams(pq_bits=bits, pq_dim=pq_dim, use_subspaces=subspaces, use_vq=vq, vq_n_centers=n_vq,
                                kmeans_n_iters=25, pq_kmeans_type=ktype, max_train_points_per_pq_code=256,
                                max_train_points_per_vq_cluster=1024)
    if n < (1 << bits) or dim % pq_dim != 0:
        with pytest.raises(CuvsError):
            pq.build(params, x)  # (the reference builds from the host copy here)
        return
    src = x if host else dev(x)
    q = pq.build(params, src)
    codes, labels = pq.transform(q, src)
    assert codes.shape == (n, q.encoded_dim) and (labels is not None) == vq
    assert codes[:50].any()
    take = min(500, n)
    rec = pq.inverse_transform(q, codes[:take].contiguous(), vq_labels=None if labels is None else labels[:take].contiguous())
    d = np.sqrt(((x[:take].astype(np.float64) - rec.cpu().numpy().astype(np.float64)) ** 2).sum(1) / dim)
    bound = 1.2 * 0.04 * 2.0 ** (8.0 * dim / (pq_dim * bits))
    print(f"{row}: max row error {d.max():.4f}, mean {d.mean():.4f}, bound {bound:.4g}")
    if dim > 5:
        assert (d <= bound).all()


# ---------------------------------------------------------------------------------------------- 6: the reference's Python tests
@pytest.mark.parametrize("n_rows", [700, 1000])
@pytest.mark.parametrize("n_cols", [64, 128])
@pytest.mark.parametrize("pq_bits", [7, 9])
@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("pq_kmeans_type", [KM, KMB])
@pytest.mark.parametrize("use_vq", [True, False])
@pytest.mark.parametrize("use_subspaces", [True, False])
@pytest.mark.parametrize("device_memory", [True, False])
def test_reference_python_grid(n_rows, n_cols, pq_bits, inplace, pq_kmeans_type, use_vq, use_subspaces, device_memory):
    input1 = np.random.default_rng(n_rows * n_cols + pq_bits).random((n_rows, n_cols)).astype(np.float32)
    input1_device = dev(input1)
    params = pq.QuantizerParams(pq_bits=pq_bits, pq_dim=32, use_subspaces=use_subspaces, use_vq=use_vq, vq_n_centers=0,
                                pq_kmeans_type=pq_kmeans_type)
    quantizer = pq.build(params, input1_device if device_memory else input1)
    output_device = torch.zeros((n_rows, quantizer.encoded_dim), dtype=torch.uint8, device="cuda") if inplace else None
    vq_labels_device = torch.zeros((n_rows,), dtype=torch.uint32, device="cuda") if inplace and use_vq else None
    if device_memory:
        transformed, vq_labels_device = pq.transform(quantizer, input1_device, codes_output=output_device, vq_labels=vq_labels_device)
    else:
        transformed, vq_labels_device = pq.transform(quantizer, input1, codes_output=output_device)
    actual = (output_device if inplace else transformed).cpu().numpy()
    assert actual.any() and bool(quantizer.pq_codebook.any())
    reconstructed = torch.empty((n_rows, n_cols), dtype=torch.float32, device="cuda")
    pq.inverse_transform(quantizer, transformed, reconstructed, vq_labels=vq_labels_device)
    assert not bool(torch.isnan(reconstructed).any())
    assert float(torch.linalg.norm(input1_device - reconstructed, dim=1).mean()) < 1.5


def test_reference_extreme_cases():
    dataset = torch.rand((5000, 2048), device="cuda", dtype=torch.float32)
    quantizer = pq.build(pq.QuantizerParams(pq_bits=8, pq_dim=2), dataset)
    codes, _ = pq.transform(quantizer, dataset)
    assert codes.shape == (5000, 2)


@pytest.mark.parametrize("use_vq", [True, False])
@pytest.mark.parametrize("use_subspaces", [True, False])
@pytest.mark.parametrize("pq_dim", [64, 128])
def test_reference_recall(use_vq, use_subspaces, pq_dim):
    rng = np.random.default_rng(pq_dim)
    dataset = rng.random((5000, 256)).astype(np.float32)
    queries = dev(rng.random((150, 256)).astype(np.float32))
    params = pq.QuantizerParams(pq_bits=8, pq_dim=pq_dim, use_subspaces=use_subspaces, use_vq=use_vq, pq_kmeans_type=KMB)
    quantizer = pq.build(params, dataset)
    transformed, vq_labels = pq.transform(quantizer, dataset)
    reconstructed = pq.inverse_transform(quantizer, transformed, vq_labels=vq_labels)
    _, indices = brute_force.search(brute_force.build(reconstructed), queries, 10)
    _, indices_gt = brute_force.search(brute_force.build(dev(dataset)), queries, 10)
    a, b = indices.cpu().numpy(), indices_gt.cpu().numpy()
    recall = np.mean([len(set(a[i]) & set(b[i])) / 10.0 for i in range(len(a))])
    print(f"recall {recall:.3f} at pq_dim {pq_dim}, vq {use_vq}, subspaces {use_subspaces}")
    assert recall > (0.5 if pq_dim == 64 else 0.75)


# ---------------------------------------------------------------------------------------------- 7: training quality
def mixture(n, dim, seed):
    rng = np.random.default_rng(seed)
    centers = rng.normal(0, 2, (40, dim))
    return (centers[rng.integers(0, 40, n)] + rng.normal(0, 1, (n, dim))).astype(np.float32)


def mse_of(q, x):
    codes, labels = pq.transform(q, dev(x))
    rec = pq.inverse_transform(q, codes, vq_labels=labels).cpu().numpy()
    return float(((x.astype(np.float64) - rec.astype(np.float64)) ** 2).sum(1).mean())


@pytest.mark.parametrize("ktype", [KM, KMB])
@pytest.mark.parametrize("pq_dim,use_vq", [(32, False), (16, True)])
def test_training_quality_against_numpy_lloyd(ktype, pq_dim, use_vq):
    """Allowed: max(e) + (max(e) - min(e)) over five seeds of the numpy Lloyd baseline (product_quantizer_ref.lloyd_pq_mse),
    for classic and balanced k-means alike. With VQ the baseline quantizes the residuals to the library's OWN VQ centres (with
    fp64 labels): the comparison covers the PQ stage only, a poor VQ fit would degrade both sides and is not seen here."""
    x = mixture(20000, 128, 3)
    params = pq.QuantizerParams(pq_bits=8, pq_dim=pq_dim, use_subspaces=True, use_vq=use_vq, vq_n_centers=64, kmeans_n_iters=25,
                                pq_kmeans_type=ktype)
    q = pq.build(params, dev(x))
    ours = mse_of(q, x)
    vq_book = q.vq_codebook.cpu().numpy() if use_vq else None  # the baseline quantizes the same residuals
    e = [P.lloyd_pq_mse(x, pq_dim, 8, 25, seed, vq_book=vq_book) for seed in range(5)]
    allowed = max(e) + (max(e) - min(e))
    print(f"{ktype} pq_dim {pq_dim} vq {use_vq}: ours {ours:.5f}, baseline {['%.5f' % v for v in e]}, allowed {allowed:.5f}")
    assert ours <= allowed


# ---------------------------------------------------------------------------------------------- 8: determinism, threads
@pytest.mark.parametrize("ktype,use_vq", [(KMB, True), (KM, False)])
def test_build_and_transform_are_deterministic(ktype, use_vq):
    x = dev(mixture(6000, 64, 5))
    params = pq.QuantizerParams(pq_bits=6, pq_dim=16, use_vq=use_vq, vq_n_centers=16, pq_kmeans_type=ktype)
    q1, q2 = pq.build(params, x), pq.build(params, x)
    assert torch.equal(q1.pq_codebook, q2.pq_codebook) and torch.equal(q1.vq_codebook, q2.vq_codebook)
    c1, l1 = pq.transform(q1, x)
    c2, l2 = pq.transform(q1, x)
    assert torch.equal(c1, c2) and (l1 is None or torch.equal(l1.view(torch.int32), l2.view(torch.int32)))


def test_four_threads_share_one_quantizer():
    case = (20000, 16, 8, 8, True, True)
    q, x, _, _, codes, labels = encode_case(case)
    xd = dev(x)
    results, errors = [None] * 4, []

    def work(t):
        try:
            r = Resources()
            c, l = pq.transform(q, xd, resources=r)
            r.sync()
            results[t] = (c.cpu().numpy(), l.cpu().numpy().astype(np.int64))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for c, l in results:
        assert np.array_equal(c, codes) and np.array_equal(l, labels)


def test_refusals():
    x = dev(mixture(600, 32, 1))
    with pytest.raises(CuvsError, match="PQ bits"):
        pq.build(pq.QuantizerParams(pq_bits=3, pq_dim=8), x)
    with pytest.raises(CuvsError, match="PQ bits"):
        pq.build(pq.QuantizerParams(pq_bits=17, pq_dim=8), x)
    with pytest.raises(CuvsError, match="divisible"):
        pq.build(pq.QuantizerParams(pq_bits=4, pq_dim=5), x)
    with pytest.raises(CuvsError, match="training samples"):
        pq.build(pq.QuantizerParams(pq_bits=10, pq_dim=8), x)
    with pytest.raises(TypeError):
        pq.build(pq.QuantizerParams(pq_bits=4, pq_dim=8), x.half())
    q = pq.build(pq.QuantizerParams(pq_bits=5, pq_dim=0), x)
    assert (q.pq_dim, q.encoded_dim) == (8, 5)  # pq_dim 0 -> ceil(dim / 4)
    with pytest.raises(CuvsError):
        pq.transform(q, x, codes_output=torch.zeros((600, 6), dtype=torch.uint8, device="cuda"))  # wrong code width
    with pytest.raises(CuvsError):
        pq.transform(q, x, codes_output=torch.zeros((599, 5), dtype=torch.uint8, device="cuda"))  # wrong row count
    with pytest.raises(CuvsError):
        pq.transform(q, x[:, :16].contiguous())
    with pytest.raises(CuvsError):
        pq.inverse_transform(q, torch.zeros((10, 5), dtype=torch.uint8, device="cuda"), output=torch.zeros((10, 32), device="cpu"))

"""GPU: the three new stages of the ScaNN build against the numpy twin (tests/scann_ref.py), the build on the reference's own
test rows, host against device rows, the files, and the parameter refusals."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import product_quantizer_ref as P
from tests import scann_ref as R

pytestmark = pytest.mark.gpu
ids = lambda c: "-".join(map(str, c))  # noqa: E731


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def scann():
    from cuvs_amd.neighbors import scann as m

    return m


# ---------------------------------------------------------------------------------------------- 6. stage AVQ
AVQ_SHAPES = [(64, 2, 1), (300, 18, 5), (700, 67, 33), (500, 130, 5), (600, 520, 5)]  # rows, dim, leaves; 520: the workspace solve
AVQ_ETAS = [0.5, 1.0, 2.0]


@functools.lru_cache(maxsize=None)
def avq_inputs(shape):
    """rows, labels with an empty leaf (the last) and a singleton leaf (the one before it) where there are 5 or more, k-means-like
    centres"""
    n, dim, n_leaves = shape
    x = R.uniform(n, dim, n + dim)
    rng = np.random.default_rng(dim)
    seeds = x[rng.choice(n, n_leaves, replace=False)].copy()
    labels = R.nearest_labels(x, seeds)
    if n_leaves >= 5:
        labels[labels == n_leaves - 1] = 0
        one = np.flatnonzero(labels == n_leaves - 2)
        labels[one[1:]] = 0
        assert (labels == n_leaves - 1).sum() == 0 and (labels == n_leaves - 2).sum() == 1
    return x, labels, seeds


@functools.lru_cache(maxsize=None)
def avq_reference(shape, eta):
    x, labels, seeds = avq_inputs(shape)
    want = R.avq_centers(x, labels, seeds, eta)[0]
    plain = R.avq_centers(x, labels, seeds, eta, np.float32)[0]
    return want, float(np.abs(plain.astype(np.float64) - want).max())


@functools.lru_cache(maxsize=None)
def avq_tolerance():
    """8 times the largest difference, over all cases of this test, between the plain fp32 numpy restatement and the fp64 twin
    (both on the CPU): the factor covers the other summation order and factorisation of the device"""
    return 8 * max(avq_reference(s, e)[1] for s in AVQ_SHAPES for e in AVQ_ETAS)


@pytest.mark.parametrize("eta", AVQ_ETAS)
@pytest.mark.parametrize("shape", AVQ_SHAPES, ids=ids)
def test_stage_avq(res, shape, eta):
    """Measured on one MI355X: the largest device error over these cases is written in DESIGN 3.1z next to the tolerance."""
    x, labels, seeds = avq_inputs(shape)
    want, _ = avq_reference(shape, eta)
    dx, dl = dev(x), dev(labels)
    got = scann().avq_centers(dx, dl, dev(seeds), eta, resources=res).cpu().numpy()
    again = scann().avq_centers(dx, dl, dev(seeds), eta, resources=res).cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("avq", shape, "eta", eta, "device error", err, "tolerance", avq_tolerance())
    assert np.isfinite(got).all() and err <= avq_tolerance()
    assert (got.view(np.uint32) == again.view(np.uint32)).all()
    n_leaves = shape[2]
    if n_leaves >= 5:
        assert (got[n_leaves - 1] == seeds[n_leaves - 1]).all()  # the empty leaf keeps its centre
    if eta == 1.0:
        chain32, _ = R.avq_means_chain32(x, labels, seeds)
        assert (got.view(np.uint32) == chain32.view(np.uint32)).all()


def test_stage_avq_in_several_leaf_batches(monkeypatch, res):
    """A workspace of 1 MiB holds the Gram matrices of 15 leaves at 130 dimensions: 33 leaves go in three batches, same bits."""
    import cuvs_amd

    shape = (700, 130, 33)
    n, dim, n_leaves = shape
    x = R.uniform(n, dim, 77)
    seeds = x[:: n // n_leaves][:n_leaves].copy()
    labels = R.nearest_labels(x, seeds)
    want = scann().avq_centers(dev(x), dev(labels), dev(seeds), 2.0, resources=res).cpu().numpy()
    monkeypatch.setenv("CUVS_AMD_WORKSPACE_MB", "1")
    small = cuvs_amd.common.Resources()
    got = scann().avq_centers(dev(x), dev(labels), dev(seeds), 2.0, resources=small).cpu().numpy()
    small.sync()
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    assert np.abs(got - R.avq_centers(x, labels, seeds, 2.0)[0]).max() <= avq_tolerance()


def test_stages_across_row_batches(res):
    """70001 rows are two batches of the 65536-row walk: the carried accumulators of AVQ (eta 1 exactly the twin's chain, eta 2
    within the tolerance of test_stage_avq) and the SOAR labels of the second batch"""
    n, dim, n_leaves = 70001, 3, 4
    x = R.uniform(n, dim, 5)
    seeds = x[[0, 20000, 40000, 69000]].copy()
    labels = R.nearest_labels(x, seeds)
    got1 = scann().avq_centers(dev(x), dev(labels), dev(seeds), 1.0, resources=res).cpu().numpy()
    # the twin's chain, vectorised over the coordinates: sequential fp32 sums in ascending row id
    want1 = seeds.copy()
    num = den = 0.0
    for c in range(n_leaves):
        rows = x[labels == c]
        acc = np.zeros(dim, np.float32)
        for r in rows:
            acc = (acc + r).astype(np.float32)
        want1[c] = (acc / np.float32(len(rows))).astype(np.float32)
        num += float(R.chain(acc[None], want1[c][None])[0])
        den += float(np.float32(np.float32(len(rows)) * R.chain(want1[c][None], want1[c][None])[0]))
    want1 = (want1 * np.float32(num / den)).astype(np.float32)
    assert (got1.view(np.uint32) == want1.view(np.uint32)).all()
    got2 = scann().avq_centers(dev(x), dev(labels), dev(seeds), 2.0, resources=res).cpu().numpy()
    err = float(np.abs(got2 - R.avq_centers(x, labels, seeds, 2.0)[0]).max())
    print("avq over two row batches, eta 2: device error", err)
    assert err <= avq_tolerance()
    soar = scann().soar_labels(dev(x), dev(got2), dev(labels), 1.0, resources=res).cpu().numpy()
    assert (soar == R.soar_labels(x, got2, labels, 1.0)).all()


def test_build_host_rows_across_batches(res):
    n, dim = 70001, 4
    x = R.uniform(n, dim, 6)
    p = scann().IndexParams(n_leaves=8, kmeans_n_rows_train=8192, pq_n_rows_train=8192, pq_dim=2, pq_bits=4, partitioning_eta=2.0,
                            reordering_bf16=True, reordering_noise_shaping_threshold=0.2)
    a = index_arrays(scann().build(p, dev(x), resources=res))
    h = index_arrays(scann().build(p, x, resources=res))
    for k in a:
        assert (a[k].view(np.uint8) == h[k].view(np.uint8)).all(), k
    assert (a["soar_labels"] == R.soar_labels(x, a["centers"], a["labels"], 1.0)).all()
    assert (a["bf16"] == R.quantize_bf16(x, 0.2)).all()


# ---------------------------------------------------------------------------------------------- 7. stage SOAR
SOAR_SHAPES = [(1, 2, 1), (257, 6, 33), (1000, 18, 33), (1000, 67, 130), (257, 130, 130), (1000, 130, 33), (257, 2, 130), (1, 18, 130),
               (1000, 6, 1)]


@functools.lru_cache(maxsize=None)
def soar_inputs(shape):
    n, dim, n_leaves = shape
    x = R.uniform(n, dim, 3 * n + dim)
    centers = R.uniform(n_leaves, dim, 5 * n_leaves + dim)
    labels = R.nearest_labels(x, centers)
    if n >= n_leaves:  # some zero residuals: a centre that is a row
        for j in np.unique(labels)[:3]:
            centers[j] = x[np.flatnonzero(labels == j)[0]]
    return x, centers, labels, R.soar_parts(x, centers, labels)


@pytest.mark.parametrize("lam", [0.0, 1.0, 1.5])
@pytest.mark.parametrize("shape", SOAR_SHAPES, ids=ids)
def test_stage_soar(res, shape, lam):
    x, centers, labels, parts = soar_inputs(shape)
    want = R.soar_labels(x, centers, labels, lam, parts)
    got = scann().soar_labels(dev(x), dev(centers), dev(labels), lam, resources=res).cpu().numpy()
    print("soar", shape, "lambda", lam, "rows that differ:", int((got != want).sum()), "zero residuals:", int((parts[3] == 0).sum()))
    assert (got == want).all()


def test_stage_soar_duplicate_centres_tie_to_the_lower_id(res):
    x, centers, labels, _ = soar_inputs((1000, 18, 33))
    centers = np.concatenate([centers, centers[5:12], centers[:2]])  # ids 33 .. 41 repeat 5 .. 11 and 0, 1: across MFMA tiles and lanes
    want = R.soar_labels(x, centers, labels, 1.0)
    got = scann().soar_labels(dev(x), dev(centers), dev(labels), 1.0, resources=res).cpu().numpy()
    assert (got == want).all() and got.max() < 33 and np.isin(got, np.r_[5:12, 0, 1]).sum() > 0


# ---------------------------------------------------------------------------------------------- 8. stage bf16
@pytest.mark.parametrize("threshold", [float("nan"), 0.2])
@pytest.mark.parametrize("dim", [1, 63, 64, 65, 200])
def test_stage_bf16(res, dim, threshold):
    x = R.uniform(50, dim, dim, -2, 2)
    x[3] = 0
    x[4] = x[4] * np.float32(0.01)  # |x| below the threshold
    x[5, : dim // 2] = R.bf16_value(R.bf16_rne_bits(x[5, : dim // 2]))
    want = R.quantize_bf16(x, threshold)
    got = scann().quantize_bf16(dev(x), threshold, resources=res).cpu().numpy()
    print("bf16 dim", dim, "threshold", threshold, "coordinates moved by noise shaping:", int((want != R.quantize_bf16(x)).sum()))
    assert got.dtype == np.int16 and (got == want).all()


# ---------------------------------------------------------------------------------------------- 9. build
N_ROWS, N_LEAVES = 4096, 32  # ann_scann.cuh:24-36: 4096 rows uniform in [0.1, 2), max(32, min(1024, n / 128)) leaves, both train sizes n
BUILD_CASES = {
    "defaults": dict(dim=64),
    **{"dim%d-bits%d" % (d, b): dict(dim=d, pq_dim=2, pq_bits=b) for b in (4, 8) for d in (2, 6, 10, 18)},
    "eta2": dict(dim=64, partitioning_eta=2.0),
    "lambda1.5": dict(dim=64, soar_lambda=1.5),
    "bf16": dict(dim=64, reordering_bf16=True),
    "bf16-avq": dict(dim=64, reordering_bf16=True, reordering_noise_shaping_threshold=0.2),
}


def build_params(kw):
    kw = dict(kw)
    kw.pop("dim")
    return scann().IndexParams(n_leaves=N_LEAVES, kmeans_n_rows_train=N_ROWS, pq_n_rows_train=N_ROWS, **kw)


def index_arrays(idx):
    out = dict(centers=idx.centers.cpu().numpy(), labels=idx.labels.cpu().numpy(), soar_labels=idx.soar_labels.cpu().numpy(),
               pq_codebook=idx.pq_codebook.cpu().numpy(), codes=idx.quantized_residuals, soar_codes=idx.quantized_soar_residuals)
    if idx.has_bf16:
        out["bf16"] = idx.bf16_dataset
    return out


@pytest.mark.parametrize("name", list(BUILD_CASES), ids=list(BUILD_CASES))
def test_build(res, name, tmp_path):
    from cuvs_amd.cluster import kmeans

    kw = BUILD_CASES[name]
    dim = kw["dim"]
    p = build_params(kw)
    pq_dim, bits = p.pq_dim, p.pq_bits
    n_sub, book_n = dim // pq_dim, 1 << bits
    x = R.uniform(N_ROWS, dim, 1234)
    dx = dev(x)
    idx = scann().build(p, dx, resources=res)
    a = index_arrays(idx)
    # the reference's shape checks (ann_scann.cuh:112-135)
    assert (idx.size, idx.dim, idx.n_leaves, idx.pq_dim, idx.pq_bits) == (N_ROWS, dim, N_LEAVES, pq_dim, bits)
    assert a["centers"].shape == (N_LEAVES, dim) and a["labels"].shape == a["soar_labels"].shape == (N_ROWS,)
    assert a["pq_codebook"].shape == (book_n, dim)
    assert a["codes"].shape == a["soar_codes"].shape == (N_ROWS, n_sub) and a["codes"].dtype == np.uint8
    assert idx.has_bf16 == bool(kw.get("reordering_bf16", False))

    # labels: the library's own balanced fit and predict on the same rows give the pre-AVQ centres and the same labels
    kp = kmeans.KMeansParams(n_clusters=N_LEAVES, hierarchical=True, hierarchical_n_iters=p.kmeans_n_iters)
    pre = kmeans.fit(kp, dx, resources=res).centroids
    labels = kmeans.predict(kp, dx, pre, resources=res).labels.cpu().numpy()
    assert (a["labels"] == labels).all()
    # centres: the stage on the pre-AVQ centres, bit for bit (the stage has its own test against the twin)
    stage = scann().avq_centers(dx, dev(labels), pre.clone(), p.partitioning_eta, resources=res).cpu().numpy()
    assert (stage.view(np.uint32) == a["centers"].view(np.uint32)).all()
    # SOAR labels: the twin on the index's own centres and labels
    want = R.soar_labels(x, a["centers"], labels, p.soar_lambda)
    print(name, "SOAR rows that differ:", int((want != a["soar_labels"]).sum()), "same leaf: %.1f %%" % (100 * (want == labels).mean()))
    assert (a["soar_labels"] == want).all()

    # codes: below 2^bits, and no worse than the fp64 argmin by more than the chain's rounding, for both residuals
    book = R.sub_books(a["pq_codebook"], pq_dim)
    allowed = 4 * (pq_dim + 2) * 2.0 ** -24
    for which, lab in (("codes", labels), ("soar_codes", a["soar_labels"])):
        codes = a[which].astype(np.int64)
        assert codes.max() < book_n
        r = P.residual(x, a["centers"], lab)
        worst, differ = P.distance_excess(r, book, codes, n_sub, pq_dim, bits, True)
        print(name, which, "codes that differ from the fp64 argmin:", differ, "worst excess", worst, "allowed", allowed)
        assert worst <= allowed
    # the reference's reconstruction test (ann_scann.cuh:253-268)
    rec = P.decode(book, a["codes"].astype(np.int64), pq_dim, bits, True, a["centers"], labels)
    rms = np.sqrt(((x - rec).astype(np.float32) ** 2).mean(1))
    print(name, "reconstruction: mean", float(rms.mean()), "max", float(rms.max()))
    assert rms.mean() < 0.95 and rms.max() < 0.95 * 1.5
    if idx.has_bf16:
        assert (a["bf16"] == R.quantize_bf16(x, p.reordering_noise_shaping_threshold)).all()
    else:
        assert idx.bf16_dataset is None

    # host rows: the same index, every array equal
    host = index_arrays(scann().build(p, x, resources=res))
    assert sorted(host) == sorted(a)
    for k in a:
        assert a[k].dtype == host[k].dtype and (a[k].view(np.uint8) == host[k].view(np.uint8)).all(), k

    # the files
    d = str(tmp_path / "scann")
    scann().save(d, idx, resources=res)
    meta = R.read_metadata(os.path.join(d, "cuvs_metadata.bin"))
    assert [m.dtype for m in meta] == [np.int32, np.uint32, np.uint32] and [int(m) for m in meta] == [1, dim, pq_dim]
    load = lambda f: np.load(os.path.join(d, f))  # noqa: E731
    assert (load("centers.npy") == a["centers"]).all() and (load("pq_codebook.npy") == a["pq_codebook"]).all()
    tok = load("datapoint_to_token.npy")
    assert tok.dtype == np.int32 and (tok == R.interleave_labels(labels, a["soar_labels"])).all()
    assert (load("hashed_dataset.npy") == a["codes"]).all() and (load("hashed_dataset_soar.npy") == a["soar_codes"]).all()
    assert load("hashed_dataset.npy").dtype == np.uint8
    if idx.has_bf16:
        b = load("bf16_dataset.npy")
        assert b.dtype == np.int16 and (b == a["bf16"]).all()
    else:
        assert not os.path.exists(os.path.join(d, "bf16_dataset.npy"))


# ---------------------------------------------------------------------------------------------- 10. refusals
@pytest.mark.parametrize("kw,rows,dtype,word", [
    (dict(pq_bits=5), 4096, np.float32, "pq_bits"),
    (dict(pq_dim=7), 4096, np.float32, "multiple of pq_dim"),
    (dict(partitioning_eta=0.0), 4096, np.float32, "partitioning_eta"),
    (dict(soar_lambda=-1.0), 4096, np.float32, "soar_lambda"),
    (dict(), 4096, np.float16, "fp32"),
    (dict(), 16, np.float32, "n_leaves"),
], ids=["pq_bits5", "dim-not-multiple", "eta0", "lambda-negative", "fp16-rows", "rows-below-leaves"])
def test_parameter_refusals(res, kw, rows, dtype, word):
    """CUVS_ERROR with a text, from checks that run before the first launch: none of the build's timed kernels is seen"""
    from cuvs_amd._lib import CuvsError, lib

    x = dev(R.uniform(rows, 64, 1).astype(dtype))
    p = scann().IndexParams(n_leaves=32, kmeans_n_rows_train=4096, pq_n_rows_train=4096, **kw)
    kernels = (b"avq_vec_kernel", b"soar_tile_kernel", b"pq_encode_kernel", b"pq_encode_plain_kernel", b"bf16_kernel")
    lib().cuvsAmdProfileEnable(1)
    try:
        for k in kernels:
            lib().cuvsAmdProfileCollect(k, None)  # reset
        with pytest.raises(CuvsError, match=word):
            scann().build(p, x, resources=res)
        assert all(lib().cuvsAmdProfileCollect(k, None) == 0 for k in kernels)
    finally:
        lib().cuvsAmdProfileEnable(0)

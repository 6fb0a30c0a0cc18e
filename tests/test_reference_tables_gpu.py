"""GPU: the reference's own IVF-PQ / IVF-Flat / CAGRA test tables (tests/golden/reference_test_tables.py, transcribed with
file:line from cpp/tests/neighbors/{ann_ivf_pq,ann_ivf_flat,ann_cagra}.cuh), every case id a test of its own, with the
reference's generators' ranges and its own pass criterion:

  * data: float rows uniform [0.1, 2.0), int8 / uint8 rows uniform integers [1, 20) (ann_ivf_pq.cuh:150-168,
    ann_ivf_flat.cuh:490-506); CAGRA: rounding-error-free rows k / 2^s in [-1, 1), unit rows for inner product
    (ann_cagra.cuh:140-199). The reference's generator is RAFT's; the stream differs, the distribution is the same.
  * ground truth: naive kNN in float (naive_knn.cuh:22-87; here float64 on the GPU, cast to float).
  * pass: eval_neighbours - a returned neighbour counts when its id OR its distance (CompareApprox eps) matches one of the
    expected k (ann_utils.cuh:114-125,222-289) - recall >= min_recall - eps, plus the uniqueness of the returned ids;
    IVF-PQ also the out-of-bounds invariants of ann_ivf_pq.cuh:658-680.

The reference holds no golden OUTPUTS for these searches: thresholds and generator ranges are the pin there is."""
import math
import os

import numpy as np
import pytest

from tests.golden import reference_test_tables as T

pytestmark = pytest.mark.gpu

DT = {"f32": np.float32, "f16": np.float16, "u8": np.uint8, "i8": np.int8}
INVALID = np.iinfo(np.int64).max


def _gen(n, dim, dtype, seed, device="cuda"):
    import torch

    g = torch.Generator(device=device)
    g.manual_seed(seed)
    if dtype in ("f32", "f16"):
        x = torch.rand((n, dim), generator=g, device=device, dtype=torch.float32) * 1.9 + 0.1
        return x.half() if dtype == "f16" else x
    x = torch.randint(1, 20, (n, dim), generator=g, device=device, dtype=torch.int32)
    return x.to(torch.int8 if dtype == "i8" else torch.uint8)


def _naive_knn(q, x, k, metric, chunk=4096):
    """naive_knn.cuh: exact distances in floating point, the k best by the metric's order. q, x: device tensors."""
    import torch

    xd = x.double()
    xn = (xd * xd).sum(1)
    out_d, out_i = [], []
    for q0 in range(0, q.shape[0], chunk):
        qd = q[q0:q0 + chunk].double()
        dot = qd @ xd.T
        if metric == "inner_product":
            d = dot
            v, i = torch.topk(d, k, dim=1, largest=True)
        else:
            if metric == "cosine":
                d = 1.0 - dot / (qd.norm(dim=1)[:, None] * xn.sqrt()[None, :])
            else:
                d = ((qd * qd).sum(1)[:, None] - 2.0 * dot + xn[None, :]).clamp_(min=0)
                if metric == "euclidean":
                    d = d.sqrt()
            v, i = torch.topk(d, k, dim=1, largest=False)
        out_d.append(v.float()); out_i.append(i)
    return torch.cat(out_d), torch.cat(out_i)


def _eval_neighbours(exp_i, act_i, exp_d, act_d, eps, min_recall, test_unique=True, chunk=65536):
    """ann_utils.cuh:222-289 on the device: match = same id OR CompareApprox(eps)(distance) (test_utils.h:41-54:
    ratio = |a-b| > eps ? |a-b| / max(|a|,|b|) : |a-b|; ratio <= eps); recall >= min_recall - eps; ids unique per row."""
    import torch

    rows, k = act_i.shape
    hits = 0
    for r0 in range(0, rows, chunk):
        ai, ad = act_i[r0:r0 + chunk, :, None], act_d[r0:r0 + chunk, :, None].double()
        ei, ed = exp_i[r0:r0 + chunk, None, :], exp_d[r0:r0 + chunk, None, :].double()
        diff = (ad - ed).abs()
        m = torch.maximum(ad.abs(), ed.abs())
        ratio = torch.where(diff > eps, diff / m, diff)
        hits += int(((ai == ei) | (ratio <= eps)).any(dim=2).sum().item())
    recall = hits / (rows * k)
    if os.environ.get("CUVS_AMD_TABLE_LOG"):   # margins of every case, for profiles/ (test id from pytest's own variable)
        with open(os.environ["CUVS_AMD_TABLE_LOG"], "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split('::')[-1].split(' ')[0]} recall {recall:.4f} min_recall {min_recall:.4f}\n")
    assert recall >= min_recall - eps, f"recall {recall:.4f} < min_recall {min_recall:.4f} (eps {eps:g})"
    if test_unique:
        s = torch.sort(act_i, dim=1).values
        dup = ((s[:, 1:] == s[:, :-1]) & (s[:, 1:] != INVALID)).sum().item()
        assert dup == 0, f"{dup} duplicate ids"
    return recall


# --------------------------------------------------------------------------------------------------------------- IVF-PQ
def _ivf_pq_params():
    out = []
    for dtype, tables in T.IVF_PQ_TABLES.items():
        for name, fn in tables:
            for n, case in enumerate(fn()):
                out.append(pytest.param(dtype, case, id=f"{dtype}-{name}-{n:02d}"))
    return out


@pytest.mark.parametrize("dtype,case", _ivf_pq_params())
def test_ivf_pq_reference_table(dtype, case, res):
    import torch
    from cuvs_amd.neighbors import ivf_pq

    c = case
    x = _gen(c["num_db_vecs"], c["dim"], dtype, 1234)
    q = _gen(c["num_queries"], c["dim"], dtype, 4321)
    ip = ivf_pq.IndexParams(n_lists=c["n_lists"], metric=c["metric"], kmeans_trainset_fraction=c["kmeans_trainset_fraction"],
                            pq_bits=c["pq_bits"], pq_dim=c["pq_dim"], codebook_kind=c["codebook_kind"],
                            force_random_rotation=c["force_random_rotation"], add_data_on_build=True)
    index = ivf_pq.build(ip, x, resources=res)
    sp = ivf_pq.SearchParams(n_probes=c["n_probes"], lut_dtype=DT[c["lut_dtype"]], internal_distance_dtype=DT[c["internal_distance_dtype"]],
                             coarse_search_dtype=DT[c["coarse_search_dtype"]])
    d, i = ivf_pq.search(sp, index, q, c["k"], resources=res)
    res.sync()
    td, ti = _naive_knn(q, x, c["k"], c["metric"])
    min_recall, eps = T.ivf_pq_min_recall(c, index.pq_dim)
    _eval_neighbours(ti, i, td, d, eps, min_recall)
    # ann_ivf_pq.cuh:658-680: out-of-bounds records only where the probed lists hold fewer than k rows; no invalid / impossible id
    sizes = np.sort(index.list_sizes.cpu().numpy().astype(np.int64))
    sizes = sizes[sizes > 0]
    min_results = int(sizes[:min(len(sizes), c["n_probes"])].sum())   # min_output_size(): the n_probes smallest non-empty lists
    max_oob = 0 if c["k"] <= min_results else c["k"] - min_results
    ih = i.cpu().numpy()
    oob = ih == INVALID
    assert int(oob.sum()) <= max_oob * ih.shape[0]
    assert ((ih[~oob] >= 0) & (ih[~oob] < c["num_db_vecs"])).all()


@pytest.mark.parametrize("case", [pytest.param(c, id=f"f32-flat_layout_tests-{n:02d}") for n, c in enumerate(T.ivf_pq_flat_layout_tests())])
def test_ivf_pq_flat_layout_codes(case, res, tmp_path):
    """check_flat_layout_codes (ann_ivf_pq.cuh:472-590) through what the C ABI exposes: a FLAT and an INTERLEAVED index with the
    same model hold the same lists, codes and ids; the FLAT one refuses to search (ivf_pq_search.cuh:914-916), its file carries
    list_layout 0 and [size, bytes_per_vector] list records (ivf_pq.hpp:302-338) and loads back as a FLAT index."""
    import sys, os
    import torch
    from cuvs_amd._lib import CuvsError
    from cuvs_amd.neighbors import ivf_pq

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import refformat

    c = case
    x = _gen(c["num_db_vecs"], c["dim"], "f32", 1234)
    q = _gen(64, c["dim"], "f32", 4321)
    ids = torch.arange(c["num_db_vecs"], dtype=torch.int64, device="cuda")
    built = {}
    for layout in ("interleaved", "flat"):
        ip = ivf_pq.IndexParams(n_lists=c["n_lists"], kmeans_trainset_fraction=1.0, pq_bits=c["pq_bits"], pq_dim=c["pq_dim"],
                                codebook_kind=c["codebook_kind"], add_data_on_build=False, codes_layout=layout)
        idx = ivf_pq.build(ip, x, resources=res)          # deterministic training: the same model for both
        ivf_pq.extend(idx, x, ids, resources=res)
        assert idx.codes_layout == layout
        built[layout] = idx
    a, b = built["interleaved"], built["flat"]
    assert torch.equal(a.list_sizes, b.list_sizes)
    codes = []
    for L in range(c["n_lists"]):
        if int(a.list_sizes[L].item()) == 0:
            codes.append(np.zeros((0, (c["pq_dim"] * c["pq_bits"] + 7) // 8), np.uint8))
            continue
        ca, cb = a.list_data(L, resources=res), b.list_data(L, resources=res)
        assert torch.equal(ca, cb) and torch.equal(a.list_indices(L), b.list_indices(L))
        codes.append(cb.cpu().numpy())
    ivf_pq.search(ivf_pq.SearchParams(n_probes=4), a, q, 5, resources=res)     # the INTERLEAVED one searches
    with pytest.raises(CuvsError, match="INTERLEAVED codes layout"):
        ivf_pq.search(ivf_pq.SearchParams(n_probes=4), b, q, 5, resources=res)
    fn = str(tmp_path / "flat.ivfpq")
    ivf_pq.save(fn, b, resources=res)
    f = refformat.parse_ivf_pq(fn)
    assert f["codes_layout"] == 0 and f["pq_bits"] == c["pq_bits"] and f["pq_dim"] == c["pq_dim"]
    sizes = a.list_sizes.cpu().numpy()
    for L in range(c["n_lists"]):   # the file's records, parsed by the independent reader, hold the codes the index hands out
        want = refformat.bitstream_to_codes(codes[L], c["pq_dim"], c["pq_bits"]) if sizes[L] else f["codes"][L]
        assert (f["codes"][L] == want).all()
    back = ivf_pq.load(fn, resources=res)
    assert back.codes_layout == "flat" and torch.equal(back.list_sizes, b.list_sizes)
    for L in range(c["n_lists"]):
        if sizes[L]:
            assert torch.equal(back.list_data(L, resources=res), b.list_data(L, resources=res))


# ------------------------------------------------------------------------------------------------------------- IVF-Flat
def _ivf_flat_params():
    out = []
    for dtype in ("f32", "f16", "i8", "u8"):   # ann_ivf_flat/test_{float,half,int8_t,uint8_t}_int64_t.cu all instantiate `inputs`
        for n, case in enumerate(T.IVF_FLAT_CASES):
            # the table is run in full for float rows; for the other row types every 4th case (same code paths, a quarter of the time)
            if dtype != "f32" and n % 4 != 0:
                continue
            out.append(pytest.param(dtype, case, id=f"{dtype}-inputs-{n:03d}"))
    return out


@pytest.mark.parametrize("dtype,case", _ivf_flat_params())
def test_ivf_flat_reference_table(dtype, case, res):
    import torch
    from cuvs_amd.neighbors import ivf_flat

    nq, n, dim, k, nprobe, nlist, metric, adaptive = case[:8]
    host = len(case) > 8 and case[8]
    x = _gen(n, dim, dtype, 1234)
    q = _gen(nq, dim, dtype, 4321)
    # ann_ivf_flat.cuh:106-160: add_data_on_build = false, trainset fraction 0.5, then extend() with the two halves - the
    # first without ids (row numbers continue), the second with explicit ids; host_dataset: the same from host memory
    ip = ivf_flat.IndexParams(n_lists=nlist, metric=metric, adaptive_centers=adaptive, add_data_on_build=False, kmeans_trainset_fraction=0.5,
                              metric_arg=0.0)
    src = x.cpu().numpy() if host else x
    index = ivf_flat.build(ip, src, resources=res)
    half = n // 2
    ivf_flat.extend(index, src[:half], None, resources=res)
    ids = np.arange(half, n, dtype=np.int64) if host else torch.arange(half, n, dtype=torch.int64, device="cuda")
    ivf_flat.extend(index, src[half:], ids, resources=res)
    d, i = ivf_flat.search(ivf_flat.SearchParams(n_probes=nprobe), index, q, k, resources=res)
    res.sync()
    td, ti = _naive_knn(q, x, k, metric, chunk=16384)
    eps = 0.005 if dtype == "f16" else 0.001   # :245
    _eval_neighbours(ti, i, td, d, eps, nprobe / nlist)


# ---------------------------------------------------------------------------------------------------------------- CAGRA
def _cagra_rows(n, dim, metric, seed):
    """ann_cagra.cuh:140-199: integers in [-r, r) over r = 2^floor((24 - log2(dim) - 1) / 2); inner product: unit rows."""
    import torch

    r = 1 << int(math.floor((24 - math.log2(dim) - 1) / 2))
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.randint(-r, r, (n, dim), generator=g, device="cuda", dtype=torch.int32).float() / r
    if metric == "inner_product":
        x = x / x.norm(dim=1, keepdim=True).clamp_min(1e-30)
    return x


def _cagra_params():
    out = []
    for n, c in enumerate(T.cagra_cases()):
        marks = []
        if c["metric"] in ("bitwise_hamming", "l1"):
            # (the reference itself skips L1 unless the build is ITERATIVE_CAGRA_SEARCH and Hamming for float rows: :335-347)
            marks.append(pytest.mark.skip(reason="metric outside this repo's scope (DESIGN 7); skipped by the reference for these rows too"))
        elif c["metric"] == "cosine" and c["dim"] == 1:
            marks.append(pytest.mark.skip(reason="the reference skips cosine at dim 1 (ann_cagra.cuh:348-353)"))
        name = f"{c['table']}-{n:03d}-{c['metric']}-{c['build_algo']}-{c['algo']}-d{c['dim']}-q{c['n_queries']}-k{c['k']}"
        out.append(pytest.param(c, id=name, marks=marks))
    return out


@pytest.mark.parametrize("c", _cagra_params())
def test_cagra_reference_table(c, res, tmp_path):
    import torch
    from cuvs_amd.neighbors import cagra

    x = _cagra_rows(c["n_rows"], c["dim"], c["metric"], 1234)
    q = _cagra_rows(c["n_queries"], c["dim"], c["metric"], 4321)
    index = cagra.build(cagra.IndexParams(metric=c["metric"], build_algo=c["build_algo"]), x, resources=res)
    # :446-455: serialize (with the dataset), deserialize, search the loaded index
    fn = str(tmp_path / "cagra_index.bin")
    cagra.save(fn, index, include_dataset=c["include_serialized_dataset"], resources=res)
    index = cagra.load(fn, resources=res)
    sp = cagra.SearchParams(algo=c["algo"], max_queries=c["max_queries"], team_size=c["team_size"])   # :413-416 (itopk_size stays at its default)
    d, i = cagra.search(sp, index, q, c["k"], resources=res)
    res.sync()
    td, ti = _naive_knn(q, x, c["k"], c["metric"])
    ii = i.to(torch.int64) & 0xFFFFFFFF if i.dtype != torch.int64 else i
    _eval_neighbours(ti, ii, td, d, 0.003, c["min_recall"])
    # eval_distances (:489-499): the returned distance is the exact distance of the returned row (1e-4)
    xd, qd = x.double(), q.double()
    rows = xd[ii.clamp(0, c["n_rows"] - 1)]
    if c["metric"] == "inner_product":
        exact = -(rows * qd[:, None, :]).sum(2) if (d < 0).any() else (rows * qd[:, None, :]).sum(2)
    elif c["metric"] == "cosine":
        exact = 1.0 - (rows * qd[:, None, :]).sum(2) / (rows.norm(dim=2) * qd.norm(dim=1)[:, None])
    else:
        exact = ((rows - qd[:, None, :]) ** 2).sum(2)
    assert torch.allclose(d.double(), exact, atol=1e-4, rtol=1e-4)


# ---------------------------------------------------------------------------------------------------------- brute force
def _match_knn_pair(exp_i, act_i, exp_d, act_d, eps):
    """knn_utils.cuh:19-70 with sort_inputs: both sides sorted by (distance, id), then position by position id OR CompareApprox."""
    import torch

    def srt(d, i):
        # lexicographic (distance, id): sort by id first, then stable by distance
        o = torch.argsort(i, dim=1, stable=True)
        d, i = torch.gather(d, 1, o), torch.gather(i, 1, o)
        o = torch.argsort(d, dim=1, stable=True)
        return torch.gather(d, 1, o), torch.gather(i, 1, o)

    ed, ei = srt(exp_d.double(), exp_i)
    ad, ai = srt(act_d.double(), act_i)
    diff = (ad - ed).abs()
    m = torch.maximum(ad.abs(), ed.abs())
    ratio = torch.where(diff > eps, diff / m, diff)
    bad = ~((ai == ei) | (ratio <= eps))
    assert not bool(bad.any()), f"{int(bad.sum())} positions differ, first at {torch.nonzero(bad)[0].tolist()}"


@pytest.mark.parametrize("case", [pytest.param(c, id=f"f32-inputs-{n:02d}") for n, c in enumerate(T.BRUTE_FORCE_CASES)])
def test_brute_force_reference_table(case, res, tmp_path):
    from cuvs_amd.neighbors import brute_force

    nq, n, dim, k, metric = case
    x = _gen(n, dim, "f32", 1234)
    q = _gen(nq, dim, "f32", 4321)
    td, ti = _naive_knn(q, x, k, {"l2_unexpanded": "sqeuclidean"}.get(metric, metric), chunk=1024 if n >= 500000 else 4096)
    index = brute_force.build(x, metric=metric, resources=res)
    d, i = brute_force.search(index, q, k, resources=res)
    res.sync()
    _match_knn_pair(ti, i, td, d, 0.001)
    fn = str(tmp_path / "bf.bin")            # :106-127: the same after serialize / deserialize
    brute_force.save(fn, index, resources=res)
    d2, i2 = brute_force.search(brute_force.load(fn, resources=res), q, k, resources=res)
    res.sync()
    _match_knn_pair(ti, i2, td, d2, 0.001)


# --------------------------------------------------------------------------------------------------------------- refine
@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("case", [pytest.param(c, id=f"inputs-{n:02d}") for n, c in enumerate(T.REFINE_CASES)])
def test_refine_reference_table(case, dtype, res):
    import torch
    from cuvs_amd.neighbors import refine

    nq, n, dim, k, k0, metric, host = case
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    if dtype == "f32":   # refine_helper.cuh:56-68
        x = torch.rand((n, dim), generator=g, device="cuda") * 20.0 - 10.0
        q = torch.rand((nq, dim), generator=g, device="cuda") * 20.0 - 10.0
    else:
        x = torch.randint(1, 20, (n, dim), generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
        q = torch.randint(1, 20, (nq, dim), generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
    _, cand = _naive_knn(q, x, k0, metric)      # the k0 exact neighbours as candidates (:70-90)
    td, ti = _naive_knn(q, x, k, metric)
    if host:
        d, i = refine(x.cpu().numpy(), q.cpu().numpy(), cand.cpu().numpy(), k=k, metric=metric, resources=res)
        d, i = torch.as_tensor(np.asarray(d)).cuda(), torch.as_tensor(np.asarray(i)).cuda()
    else:
        d, i = refine(x, q, cand, k=k, metric=metric, resources=res)
        res.sync()
    _eval_neighbours(ti, i, td, d, 0.001, 1.0)


# ----------------------------------------------------------------------------------------------------------- NN-descent
def _nn_descent_params():
    out = []
    for n, c in enumerate(T.NN_DESCENT_CASES):
        marks = [pytest.mark.skip(reason="metric outside this repo's scope (DESIGN 7)")] if c[3] in ("bitwise_hamming", "l1") else []
        out.append(pytest.param(c, id=f"f32-inputs-{n:03d}-{c[3]}-n{c[0]}-d{c[1]}-deg{c[2]}-{'host' if c[4] else 'device'}", marks=marks))
    return out


@pytest.mark.parametrize("case", _nn_descent_params())
def test_nn_descent_reference_table(case, res):
    import torch
    from cuvs_amd.neighbors import nn_descent

    n, dim, degree, metric, host, min_recall = case
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    x = torch.randn((n, dim), generator=g, device="cuda") * 2.0 + 0.1    # N(0.1, 2.0): ann_nn_descent.cuh:162-164
    index = nn_descent.build(nn_descent.IndexParams(metric=metric, graph_degree=degree, intermediate_graph_degree=2 * degree, max_iterations=100),   # :108-112
                             x.cpu().numpy() if host else x, resources=res)
    graph = index.graph.to(torch.int64) & 0xFFFFFFFF
    dist = index.distances
    td, ti = _naive_knn(x, x, degree, metric)     # the exact kNN graph (a row is its own nearest neighbour, as in the reference)
    _eval_neighbours(ti, graph, td, dist, 0.001, min_recall, test_unique=False)


def _nn_descent_typed_params():
    out = []
    for n, c in enumerate(T.NN_DESCENT_TYPED_CASES):
        marks = [pytest.mark.skip(reason="metric outside this repo's scope (DESIGN 7)")] if c[4] == "l1" else []
        out.append(pytest.param(c, id=f"{c[0]}-inputs-{n:03d}-{c[4]}-n{c[1]}-d{c[2]}-deg{c[3]}-{'host' if c[5] else 'device'}", marks=marks))
    return out


@pytest.mark.parametrize("case", _nn_descent_typed_params())
def test_nn_descent_reference_table_typed_rows(case, res):
    """The table above for int8 / uint8 rows (the reference's generators: uniform integers [-5, 5) / [0, 5), seed 1234) and for
    f16 rows (the float inputs rounded to half - exact in fp32, so the exact graph is that of the rounded values)."""
    import torch
    from cuvs_amd.neighbors import nn_descent

    dt, n, dim, degree, metric, host, min_recall = case
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    if dt == "f16":
        x = (torch.randn((n, dim), generator=g, device="cuda") * 2.0 + 0.1).half()
    else:
        lo, hi, tdt = (-5, 5, torch.int8) if dt == "i8" else (0, 5, torch.uint8)
        x = torch.randint(lo, hi, (n, dim), generator=g, device="cuda", dtype=torch.int32).to(tdt)
    index = nn_descent.build(nn_descent.IndexParams(metric=metric, graph_degree=degree, intermediate_graph_degree=2 * degree, max_iterations=100),
                             x.cpu().numpy() if host else x, resources=res)
    graph = index.graph.to(torch.int64) & 0xFFFFFFFF
    dist = index.distances
    td, ti = _naive_knn(x, x, degree, metric)
    _eval_neighbours(ti, graph, td, dist, 0.001, min_recall)   # with the uniqueness of a row's ids: n > degree, every slot is valid

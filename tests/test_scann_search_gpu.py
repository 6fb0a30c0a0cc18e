"""GPU: the ScaNN search against the numpy twin (tests/scann_search_ref.py): the approximate stage within the derived fp32 bound,
probe selection, the re-rank bit for bit, the refusals and two threads racing the lazy list build."""
import functools
import threading

import numpy as np
import pytest
import torch

from tests import scann_ref as R
from tests import scann_search_ref as S

pytestmark = pytest.mark.gpu
ids = lambda c: "-".join(map(str, c))  # noqa: E731
METRICS = [S.L2, S.IP]


def scann():
    from cuvs_amd.neighbors import scann as m

    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def built(case, metric, bf16=False):
    """(index, its arrays on the host, rows, 70 queries); zero-mean data, so that |q - c|^2 is of the size of |q|^2 and |c|^2"""
    import cuvs_amd

    n, dim, pq_dim, bits, n_leaves = case
    x = R.uniform(n, dim, n + dim, -1.0, 1.0)
    q = R.uniform(70, dim, dim, -1.0, 1.0)
    p = scann().IndexParams(metric=metric, n_leaves=n_leaves, kmeans_n_rows_train=n, pq_n_rows_train=n, pq_dim=pq_dim, pq_bits=bits,
                            kmeans_n_iters=8, reordering_bf16=bf16)
    idx = scann().build(p, dev(x), resources=cuvs_amd.common.Resources())
    a = dict(centers=idx.centers.cpu().numpy(), labels=idx.labels.cpu().numpy(), soar_labels=idx.soar_labels.cpu().numpy(),
             pq_codebook=idx.pq_codebook.cpu().numpy(), codes=idx.quantized_residuals, soar_codes=idx.quantized_soar_residuals)
    if bf16:
        a["bf16"] = idx.bf16_dataset
    return idx, a, x, q


def search(res, idx, q, k, n_probes, n_reorder=0):
    d, i = scann().search(scann().SearchParams(n_probes=n_probes, n_reorder=n_reorder), idx, dev(q), k, resources=res)
    return d.cpu().numpy(), i.cpu().numpy(), scann().search_last_stats()


# rows, dim, pq_dim, bits, leaves: K padding and ragged leaves at 4 and 8 bits; a subspace width that straddles a lane's 8
# dimensions; a codebook beyond the LDS budget; tiny and empty leaves; and the remaining decode paths (width 4 above, 1 and 24 here)
CASES = [(1500, 18, 2, 4, 32), (1500, 18, 2, 8, 32), (1200, 18, 3, 8, 32), (2000, 160, 8, 8, 32), (600, 32, 4, 8, 130),
         (700, 16, 1, 4, 32), (700, 48, 24, 4, 32)]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_approximate_stage_against_the_twin(res, case, metric):
    n, dim, pq_dim, bits, n_leaves = case
    idx, a, _, q = built(case, metric)
    rows, _, score, tol = S.entry_scores(q, a, metric, pq_dim)
    sign = 1.0 if metric == S.L2 else -1.0
    best, slack = S.row_scores(rows, sign * score, tol, n)
    n_two = int((a["labels"] != a["soar_labels"]).sum())
    sizes = np.bincount(np.concatenate([a["labels"], a["soar_labels"][a["labels"] != a["soar_labels"]]]), minlength=n_leaves)
    print(case, metric, "rows in two leaves", n_two, "leaf sizes min", sizes.min(), "max", sizes.max(), "empty", int((sizes == 0).sum()))
    for nq in (1, 33, 70):
        d, i, stats = search(res, idx, q[:nq], n, n_leaves)
        assert (np.sort(i, 1) == np.arange(n)).all()  # every row once
        err = np.abs(sign * d - np.take_along_axis(best[:nq], i, 1))
        bound = np.take_along_axis(slack[:nq], i, 1)
        print("  queries", nq, "largest error / bound", float((err / bound).max()), "stats", stats)
        assert (err <= bound).all()
        assert (np.diff(sign * d, axis=1) >= 0).all()
        assert stats[1] == nq * len(rows) and stats[3] == nq * n_two and stats[0] > 0
        assert (stats[2] > 0) == (case[1] == 160)
        # k = 10: nothing worse than the twin's 10th score by more than the bound, nothing better than it left out
        d10, i10, _ = search(res, idx, q[:nq], 10, n_leaves)
        for r in range(nq):
            assert len(set(i10[r])) == 10
            kth = np.sort(best[r])[9]
            assert (best[r, i10[r]] <= kth + slack[r, i10[r]]).all()
            out = np.setdiff1d(np.arange(n), i10[r])
            assert (best[r, out] >= kth - slack[r, out]).all()


@pytest.mark.parametrize("metric", METRICS)
def test_probe_selection(res, metric):
    case = CASES[1]
    idx, a, _, q = built(case, metric)
    c = S.coarse(q, a["centers"], metric) * (1.0 if metric == S.L2 else -1.0)
    ranked = np.sort(c, 1)
    # the coarse distance errs by about dim 2^-24 of its terms (1e-5 here): queries whose third and fourth leaf are 1e-3 apart
    sure = np.flatnonzero(ranked[:, 3] - ranked[:, 2] > 1e-3)
    assert len(sure) >= 20
    _, i, stats = search(res, idx, q[sure], 10, 3)
    top3 = np.argsort(c[sure], 1)[:, :3]
    for r in range(len(sure)):
        in_top = np.isin(a["labels"][i[r]], top3[r]) | np.isin(a["soar_labels"][i[r]], top3[r])
        assert in_top.all()
    assert stats[0] <= 3 * len(sure)


@pytest.mark.parametrize("metric", METRICS)
def test_rerank_bit_for_bit(res, metric):
    case = (1500, 70, 2, 8, 32)  # 70 dimensions: a full step of the chain and a ragged one
    n = case[0]
    idx, a, _, q = built(case, metric, True)
    for k in (1, 10, 64):
        d, i, _ = search(res, idx, q[:5], k, case[4], n_reorder=2000)
        for r in range(5):
            want_i, want_d = S.rerank(q[r], a["bf16"], np.arange(n), metric, k)
            assert (i[r] == want_i).all() and (d[r].view(np.uint32) == want_d.view(np.uint32)).all()


@pytest.mark.parametrize("what,word", [("no-bf16", "reordering_bf16"), ("k-above-reorder", "n_reorder"), ("dim", "columns"), ("metric", "metric")])
def test_refusals(res, what, word):
    from cuvs_amd._lib import CuvsError

    case = CASES[1]
    idx, _, _, q = built(case, "cosine" if what == "metric" else S.L2, what == "k-above-reorder")
    kw = dict(n_reorder=100) if what == "no-bf16" else dict(n_reorder=5) if what == "k-above-reorder" else {}
    with pytest.raises(CuvsError, match=word):
        search(res, idx, q[:, :17] if what == "dim" else q, 10, 8, **kw)


def test_two_threads_race_the_list_build(res):
    import cuvs_amd

    case = (1400, 18, 2, 8, 32)  # an index of its own: no search has built its lists
    idx, _, _, q = built(case, S.L2, True)
    out = [None, None]

    def run(t):
        out[t] = search(cuvs_amd.common.Resources(), idx, q, 10, 8, n_reorder=50)[:2]

    threads = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    d, i, _ = search(res, idx, q, 10, 8, n_reorder=50)
    for t in range(2):
        assert (out[t][1] == i).all() and (out[t][0].view(np.uint32) == d.view(np.uint32)).all()

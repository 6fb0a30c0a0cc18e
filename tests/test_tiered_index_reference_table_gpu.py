"""GPU: the reference's own test table of the tiered index (cpp/tests/neighbors/tiered_index.cu:210-219, committed as
tests/golden/tiered_index_reference_table.json), every case for the three ANN algos, judged by the reference's eval_neighbours
as tests/test_reference_tables_gpu.py restates it. The thresholds are the reference's, not tuned here."""
import itertools
import json
import os

import numpy as np
import pytest

from tests.test_reference_tables_gpu import _eval_neighbours, _naive_knn

pytestmark = pytest.mark.gpu

TABLE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiered_index_reference_table.json")))
CASES = list(itertools.product(*[TABLE["product"][f] for f in TABLE["fields"]]))


def _min_recall(algo):
    from cuvs_amd.neighbors import ivf_flat, ivf_pq

    if algo == "cagra":
        return TABLE["min_recall"]["cagra"]
    mod = ivf_flat if algo == "ivf_flat" else ivf_pq  # tiered_index.cu:107-116: the default parameters of both structs
    return mod.SearchParams().n_probes / mod.IndexParams()._p.contents.n_lists


@pytest.mark.parametrize("algo", TABLE["algos"])
@pytest.mark.parametrize("n_rows,dim,metric,k,n_queries,strategy", CASES)
def test_tiered_index_reference_table(res, n_rows, dim, metric, k, n_queries, strategy, algo):
    import torch

    from cuvs_amd.neighbors import tiered_index as T

    rng = np.random.default_rng(TABLE["data"]["seed"])
    mean, std = TABLE["data"]["mean"], TABLE["data"]["stddev"]
    rows = torch.from_numpy(rng.normal(mean, std, size=(n_rows, dim)).astype(np.float32)).cuda()
    q = torch.from_numpy(rng.normal(mean, std, size=(n_queries, dim)).astype(np.float32)).cuda()
    params = T.IndexParams(metric=metric, algo=algo, min_ann_rows=TABLE["build_params"]["min_ann_rows"],
                           create_ann_index_on_extend=TABLE["build_params"]["create_ann_index_on_extend"])
    half = n_rows // 2
    idx = T.build(params, rows[:half], resources=res)
    if strategy == "TEST_EXTEND":
        for i in range(half, n_rows):
            T.extend(idx, rows[i:i + 1], resources=res)
        final = idx
    else:
        second = T.build(params, rows[half:], resources=res)
        final = T.merge(params, [idx, second], resources=res)
    size, ann_rows, _, _ = T.info(final)
    assert size == n_rows
    # 2000 rows never pass min_ann_rows in either strategy (all tail); 4000 rows do: at row 2001 of the extends, or in the merge
    assert ann_rows == (0 if n_rows == 2000 else (2001 if strategy == "TEST_EXTEND" else 4000))
    d, i = T.search(None, final, q, k, resources=res)
    exp_d, exp_i = _naive_knn(q, rows, k, metric)
    _eval_neighbours(exp_i, i, exp_d, d, TABLE["eps"], _min_recall(algo))

"""Random ball cover at 1M rows: build, knn_query with 10k queries, all_knn_query's search with the 1M rows as
queries, k = 10, in 2-D and 3-D (euclidean) and 2-D (haversine), next to cuvs_amd.neighbors.brute_force on the same rows with
the L2Sqrt metric. Brute force has no haversine: there the comparator is the same index with one landmark, which scores every
row.

HIP events around each call, 2 warm-up calls, the median of --reps timed ones (1 warm-up and 3 timed for the calls that
take seconds). Reported per run: build ms, search ms, queries per second, lists visited and rows scored per query (the
library's counters), and the bytes the search loads and stores, from the counters, over the search time, in two parts:

    list bytes     = rows scored * (4 dim + 4)             the rows of the windows and, for the ones that are kept, an id
                   + lists visited * 2 * 64 * 4            the probes of the two 64-ary searches
                   + queries * (4 dim + 12 k)              the query and its result
    landmark bytes = queries * 2 * n_landmarks * (4 dim + 12)   the landmark pass, twice (radius and list bounds the second
                                                                time); every query reads the same few KB: cache traffic, not HBM

These are whole-call rates (they include the counters' read-back), not a kernel's share of peak. The first 200 queries are also
checked against an fp64 evaluation in torch (euclidean), and brute force with them: its L2Sqrt is the expanded form in fp32.

    python scripts/bench_ball_cover.py [--rows 1000000] [--queries 10000] [--k 10] [--reps 5] [--bf-self 100000] [--out FILE.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cuvs_amd.common import Resources  # noqa: E402
from cuvs_amd.neighbors import ball_cover as BC  # noqa: E402
from cuvs_amd.neighbors import brute_force  # noqa: E402


def blobs(rows, dim, seed, haversine=False):
    """the reference test's shape: Gaussian blobs; for haversine in degrees, converted to radians"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    centers = 1000
    if haversine:
        c = torch.stack([torch.rand(centers, device="cuda", generator=g) * 120 - 60, torch.rand(centers, device="cuda", generator=g) * 340 - 170], 1)
        x = c[torch.randint(0, centers, (rows,), device="cuda", generator=g)] + torch.randn(rows, 2, device="cuda", generator=g)
        return (x * (math.pi / 180.0)).float().contiguous()
    c = torch.rand(centers, dim, device="cuda", generator=g) * 20 - 10
    return (c[torch.randint(0, centers, (rows,), device="cuda", generator=g)] + 0.1 * torch.randn(rows, dim, device="cuda", generator=g)).contiguous()


def timed(fn, res, reps, warm=2):
    for _ in range(warm):
        fn()
    res.sync()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def search_bytes(stats, nq, n_landmarks, dim, k):
    """(list bytes, landmark bytes)"""
    return (stats["points_scored"] * (4 * dim + 4) + stats["lists_visited"] * 2 * 64 * 4 + nq * (4 * dim + 12 * k),
            nq * 2 * n_landmarks * (4 * dim + 12))


def fp64_ids(x, q, k):
    d = torch.cdist(q.double(), x.double())
    return torch.sort(d, dim=1, stable=True)[1][:, :k]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bf-self", type=int, default=100000, help="queries of the brute-force comparator of the self query (its time per query is reported)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    res = Resources()
    n, k = args.rows, args.k
    results = []

    def emit(row):
        results.append(row)
        print(json.dumps(row), flush=True)

    for metric, dim in (("euclidean", 2), ("euclidean", 3), ("haversine", 2)):
        x = blobs(n, dim, 10 * dim, metric == "haversine")
        q_small = blobs(args.queries, dim, 10 * dim + 1, metric == "haversine")
        params = BC.IndexParams(metric=metric)
        holder = {}

        def build():
            holder["ix"] = BC.build(params, x, resources=res)

        med, lo, hi = timed(build, res, 3, warm=1)
        ix = holder["ix"]
        L = ix.n_landmarks
        emit(dict(metric=metric, shape=f"{n}x{dim}", what="build", n_landmarks=L, median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3)))
        for what, q, reps, warm in (("knn_query", q_small, args.reps, 2), ("self_query", x, 3, 1)):
            nq = q.shape[0]
            nb = torch.empty((nq, k), dtype=torch.int64, device="cuda")
            ds = torch.empty((nq, k), dtype=torch.float32, device="cuda")
            med, lo, hi = timed(lambda: BC.knn_query(ix, q, k, neighbors=nb, distances=ds, resources=res), res, reps, warm)
            st = BC.last_stats()
            list_bytes, landmark_bytes = search_bytes(st, nq, L, dim, k)
            row = dict(metric=metric, shape=f"{n}x{dim}", what=what, queries=nq, k=k, n_landmarks=L, median_ms=round(med, 3), min_ms=round(lo, 3),
                       max_ms=round(hi, 3), queries_per_s=round(nq / med * 1e3), lists_per_query=round(st["lists_visited"] / nq, 2),
                       rows_scored_per_query=round(st["points_scored"] / nq, 1), rows_skipped_per_query=round(st["points_skipped"] / nq, 1),
                       list_bytes=list_bytes, list_gb_per_s=round(list_bytes / med / 1e6, 2), landmark_bytes=landmark_bytes,
                       landmark_gb_per_s=round(landmark_bytes / med / 1e6, 2))
            if metric == "euclidean":  # the comparator: brute force, L2Sqrt, the same rows
                nbf = nq if what == "knn_query" else min(nq, args.bf_self)
                bf = brute_force.build(x, metric="euclidean", resources=res)
                qb = q[:nbf].contiguous()
                bmed, blo, bhi = timed(lambda: brute_force.search(bf, qb, k, resources=res), res, 3, warm=1)
                row.update(brute_force_queries=nbf, brute_force_median_ms=round(bmed, 3), brute_force_queries_per_s=round(nbf / bmed * 1e3),
                           speedup_per_query=round((bmed / nbf) / (med / nq), 2))
                bd, bi = brute_force.search(bf, qb[:200], k, resources=res)
                res.sync()
                want = fp64_ids(x, q[:200], k)
                row["ids_equal_fp64_first_200"] = round(float((nb[:200] == want).float().mean()), 4)
                row["brute_force_ids_equal_fp64_first_200"] = round(float((bi == want).float().mean()), 4)
                del bf
            elif what == "knn_query":  # the comparator: one landmark, every row scored
                one = BC.build(BC.IndexParams(metric=metric, n_landmarks=1), x, resources=res)
                nb1 = torch.empty((nq, 1), dtype=torch.int64, device="cuda")
                ds1 = torch.empty((nq, 1), dtype=torch.float32, device="cuda")
                omed, olo, ohi = timed(lambda: BC.knn_query(one, q, 1, neighbors=nb1, distances=ds1, resources=res), res, 3, warm=1)
                BC.knn_query(ix, q, 1, neighbors=nb1, distances=ds1, resources=res)
                res.sync()
                imed, _, _ = timed(lambda: BC.knn_query(ix, q, 1, neighbors=nb1, distances=ds1, resources=res), res, 3, warm=1)
                row.update(one_landmark_k1_median_ms=round(omed, 3), index_k1_median_ms=round(imed, 3), speedup_k1=round(omed / imed, 2))
                del one
            emit(row)
        del ix, holder, x
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(results=results), f, indent=1)


if __name__ == "__main__":
    main()

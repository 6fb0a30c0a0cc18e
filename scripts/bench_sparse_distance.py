"""Sparse (CSR) pairwise distances and sparse brute-force kNN on two shapes: TF-IDF-like rows (n_cols 100k,
100 entries per row, columns drawn from a Zipf-like law) and a narrow matrix (n_cols 4096, 5 % dense); cosine (intersection
family) and L1 (union family), kNN with k = 10, next to the one thing a caller had before: densify both operands and call
pairwise_distance (cosine only; the dense path has no L1).

HIP events around each call, --warmup calls first, the median of --reps timed ones. Every time is also given against the
floor written down before the first run (profiles/sparse_distance_bench.md): every (entry of y, tile of four x rows) visit
reads 8 bytes of y and, in the intersection kernel, 16 bytes of LDS per lane.

    python scripts/bench_sparse_distance.py [--rows 20000] [--reps 5] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cuvs_amd.common import Resources  # noqa: E402
from cuvs_amd.distance import pairwise_distance, set_sparse_walk_form, sparse_last_stats, sparse_pairwise_distance  # noqa: E402
from cuvs_amd.neighbors import sparse_brute_force  # noqa: E402

FORMS = (1, 2, 3, 4, 0)
LDS_BYTES_PER_S = 256 * 256 * 2.4e9   # 256 B / clk / CU
INFINITY_CACHE_BYTES_PER_S = 8.6e12   # gathered rows out of the Infinity Cache
L2_BYTES_PER_S = 17e12                # rows every workgroup shares, out of the XCD's L2


def tfidf_like(rows, n_cols, per_row, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    weight = 1.0 / (torch.arange(n_cols, device="cuda", dtype=torch.float32) + 10.0)
    cols = []
    for r0 in range(0, rows, 1000):
        cnt = min(1000, rows - r0)
        cols.append(torch.multinomial(weight.expand(cnt, n_cols), per_row, replacement=False, generator=g))
    cols = torch.sort(torch.cat(cols), dim=1).values.to(torch.int32)
    data = torch.rand(rows * per_row, device="cuda", generator=g) + 0.05
    indptr = torch.arange(rows + 1, device="cuda", dtype=torch.int32) * per_row
    return (indptr, cols.reshape(-1).contiguous(), data, (rows, n_cols))


def narrow(rows, n_cols, density, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    dense = torch.rand(rows, n_cols, device="cuda", generator=g)
    dense = torch.where(dense < density, dense / density + 0.05, torch.zeros_like(dense))
    nz = dense != 0
    indptr = torch.cat([torch.zeros(1, device="cuda", dtype=torch.int64), nz.sum(dim=1).cumsum(0)]).to(torch.int32)
    idx = nz.nonzero()
    return (indptr, idx[:, 1].to(torch.int32).contiguous(), dense[nz].contiguous(), (rows, n_cols)), dense


def timed(fn, res, warmup, reps):
    for _ in range(warmup):
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
    return dict(median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times))


def floors(x, y, isect):
    m, nnz_y = x[3][0], int(y[1].numel())
    visits = (m + 3) // 4 * nnz_y
    out = dict(visits=visits, y_bytes_l2_ms=visits * 8 / L2_BYTES_PER_S * 1e3, y_bytes_infinity_cache_ms=visits * 8 / INFINITY_CACHE_BYTES_PER_S * 1e3)
    if isect:
        out["lds_reads_ms"] = visits * 16 / LDS_BYTES_PER_S * 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = Resources()
    n = args.rows
    results = []

    def record(shape, what, fn, **more):
        r = dict(shape=shape, what=what, **timed(fn, res, args.warmup, args.reps), **more)
        print(json.dumps(r), flush=True)
        results.append(r)

    x = tfidf_like(n, 100000, 100, 1)
    y = tfidf_like(n, 100000, 100, 2)
    out = torch.empty((n, n), dtype=torch.float32, device="cuda")
    for form in FORMS:  # 0: chosen by shape (what a caller gets); 1 - 4: every form of the walk, as comparators
        set_sparse_walk_form(form, form)
        for metric, isect in (("cosine", True), ("l1", False)):
            record("tfidf %dx%dx100000" % (n, n), "sparse %s form %d" % (metric, form),
                   lambda: sparse_pairwise_distance(x, y, out=out, metric=metric, resources=res), floor=floors(x, y, isect))
            results[-1]["stats"] = sparse_last_stats()
    set_sparse_walk_form(0, 0)
    index = sparse_brute_force.build(y, metric="cosine", resources=res)
    nb = torch.empty((n, 10), dtype=torch.int64, device="cuda")
    ds = torch.empty((n, 10), dtype=torch.float32, device="cuda")
    record("tfidf %dx%dx100000" % (n, n), "sparse kNN cosine k=10",
           lambda: sparse_brute_force.search(index, x, 10, neighbors=nb, distances=ds, resources=res))
    del x, y, index

    (xs, xd), (ys, yd) = narrow(n, 4096, 0.05, 3), narrow(n, 4096, 0.05, 4)
    for form in FORMS:
        set_sparse_walk_form(form, form)
        for metric, isect in (("cosine", True), ("l1", False)):
            record("narrow %dx%dx4096" % (n, n), "sparse %s form %d" % (metric, form),
                   lambda: sparse_pairwise_distance(xs, ys, out=out, metric=metric, resources=res), floor=floors(xs, ys, isect))
    set_sparse_walk_form(0, 0)
    record("narrow %dx%dx4096" % (n, n), "densified pairwise_distance cosine (operands already dense)",
           lambda: pairwise_distance(xd, yd, out=out, metric="cosine", resources=res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

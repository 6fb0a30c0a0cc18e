"""Single-linkage clustering: time per phase of cuvs_amd.cluster.agglomerative at
  PAIRWISE             50 000 x 64
  KNN_GRAPH         1 000 000 x 16, c = 15
  mutual reachability 1 000 000 x 16, min_samples = 15
next to the only yardstick the library had before it: the degrees-only epsilon neighbourhood of the rows against themselves
(cuvsAmdEpsNeighbors(x, x), the same 128 x 128 pair tile with a cheaper epilogue) on the same shape.

The phases come from the library's own event pairs (cuvsAmdProfileEnable / cuvsAmdProfileCollect): kNN, symmetrise, sparse
rounds (with the re-weighting), every dense round, the tile kernel inside the dense rounds, the sort by key, the host's
union-find, the labels. One warm-up call per configuration, then --reps timed calls; the median call is reported, with
its phases. Rows are blobs far apart, so that the kNN graph has components to connect.

    python scripts/single_linkage_bench.py [--configs pairwise,knn_graph,mutual_reachability] [--scale 1.0] [--reps 3] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cuvs_amd._lib import lib  # noqa: E402
from cuvs_amd.cluster import agglomerative as A  # noqa: E402
from cuvs_amd.common import Resources  # noqa: E402
from cuvs_amd.neighbors import epsilon_neighborhood as E  # noqa: E402

PHASES = ["sl_knn", "sl_symmetrise", "sl_sparse_rounds", "sl_tile_kernel", "sl_sort", "sl_dendrogram", "sl_labels"]
CONFIGS = {
    "pairwise": dict(rows=50000, dim=64, kw=dict(linkage="pairwise")),
    "knn_graph": dict(rows=1000000, dim=16, kw=dict(linkage="knn_graph", c=15)),
    "mutual_reachability": dict(rows=1000000, dim=16, kw=dict(space="mutual_reachability", min_samples=15)),
}


def blobs(rows, dim, centers, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    c = torch.rand(centers, dim, device="cuda", generator=g) * 20 - 10
    labels = torch.randperm(rows, device="cuda", generator=g) % centers
    return (c[labels] + 0.01 * torch.randn(rows, dim, device="cuda", generator=g)).contiguous()


def collect(name):
    total = C.c_double(0)
    count = lib().cuvsAmdProfileCollect(name.encode(), C.byref(total))
    return count, total.value


def wall(fn, res):
    res.sync()
    t0 = time.perf_counter()
    out = fn()
    res.sync()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="pairwise,knn_graph,mutual_reachability")
    ap.add_argument("--scale", type=float, default=1.0, help="factor on the row counts (a rehearsal at a small size)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--centers", type=int, default=100)
    ap.add_argument("--n-clusters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    res = Resources()
    lib().cuvsAmdProfileCollect.restype = C.c_int
    results = []
    for name in args.configs.split(","):
        cfg = CONFIGS[name]
        n, dim = max(2, int(cfg["rows"] * args.scale)), cfg["dim"]
        x = blobs(n, dim, min(args.centers, n), dim)

        def one_call():
            out = A.build_linkage(x, metric="sqeuclidean", resources=res, **cfg["kw"])
            return out

        def labels_call():
            return A.single_linkage(x, args.n_clusters, metric="sqeuclidean", resources=res,
                                    **{k: v for k, v in cfg["kw"].items() if k in ("linkage", "c")})

        wall(one_call, res)  # warm-up: code objects, scratch
        runs = []
        for _ in range(args.reps):
            lib().cuvsAmdProfileEnable(1)
            ms, _ = wall(one_call, res)
            stats = A.last_stats()
            phases = {p: round(collect(p)[1], 3) for p in PHASES}
            rounds = [round(collect(f"sl_dense_round_{r}")[1], 3) for r in range(stats["dense_rounds"])]
            lib().cuvsAmdProfileEnable(0)
            runs.append(dict(total_ms=round(ms, 3), phases_ms=phases, dense_round_ms=rounds, stats=stats))
        runs.sort(key=lambda r: r["total_ms"])
        row = dict(config=name, shape=f"{n}x{dim}", reps=args.reps, **runs[len(runs) // 2],
                   min_total_ms=runs[0]["total_ms"], max_total_ms=runs[-1]["total_ms"])
        if name != "mutual_reachability":  # labels: the single_linkage call (distance space) with the events of its label phase
            lib().cuvsAmdProfileEnable(1)
            ms, _ = wall(labels_call, res)
            row["single_linkage_total_ms"] = round(ms, 3)
            row["phases_ms"]["sl_labels"] = round(collect("sl_labels")[1], 3)
            for p in PHASES + [f"sl_dense_round_{r}" for r in range(64)]:
                collect(p)
            lib().cuvsAmdProfileEnable(0)
        # the yardstick: degrees only, the same pair tile
        vd = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        eps_ms = []
        wall(lambda: E.compute(x, x, 4.0, adj=False, vd=vd, resources=res), res)
        for _ in range(max(args.reps, 3)):
            eps_ms.append(wall(lambda: E.compute(x, x, 4.0, adj=False, vd=vd, resources=res), res)[0])
        row["eps_degrees_only_ms"] = round(statistics.median(eps_ms), 3)
        if row["dense_round_ms"]:
            row["dense_round_over_eps"] = round(statistics.median(row["dense_round_ms"]) / row["eps_degrees_only_ms"], 3)
        results.append(row)
        print(json.dumps(row), flush=True)
        del x, vd
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(results=results), f, indent=1)


if __name__ == "__main__":
    main()

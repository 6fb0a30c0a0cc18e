"""CAGRA search over a VPQ-compressed dataset against the uncompressed search over THE SAME graph, on one corpus of bench.py's
latent-cloud generator (fp16 rows). Prints one JSON line: per pq_len the build time with and without compression, the bytes
of the compressed dataset (checked against n * row_len + the two fp16 books), and per walk (single_cta, multi_cta) the median
ms per batch and recall@10 against fp64 ground truth for the compressed index and for an uncompressed index made from the
compressed index's graph and the original rows.

    python scripts/bench_cagra_vpq.py [--rows 1000000] [--dim 768] [--batch 10000] [--degree 64] [--itopk 64] [--reps 10]

Every timed search runs after --warmup untimed ones, with the device synchronised before and after."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def exact_topk_fp64(x, q, k, chunk=100000):
    """ids of the k nearest rows by squared L2 in float64, rows taken a chunk at a time"""
    q64 = q.double()
    best_d = torch.full((q.shape[0], k), float("inf"), dtype=torch.float64, device=q.device)
    best_i = torch.zeros((q.shape[0], k), dtype=torch.int64, device=q.device)
    for r0 in range(0, x.shape[0], chunk):
        c = x[r0:r0 + chunk].double()
        d = (c * c).sum(1)[None, :] - 2.0 * q64 @ c.T
        dd, ii = torch.topk(d, min(k, c.shape[0]), dim=1, largest=False)
        cat_d, cat_i = torch.cat([best_d, dd], 1), torch.cat([best_i, ii + r0], 1)
        best_d, pos = torch.topk(cat_d, k, dim=1, largest=False)
        best_i = torch.gather(cat_i, 1, pos)
    return best_i.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=10000)
    ap.add_argument("--degree", type=int, default=64)
    ap.add_argument("--itopk", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pq-lens", type=int, nargs="+", default=[4, 2])
    args = ap.parse_args()
    from bench import gen_rows
    from cuvs_amd.common import Resources
    from cuvs_amd.neighbors import cagra

    dev = torch.device("cuda")
    res = Resources()
    x = torch.empty((args.rows, args.dim), dtype=torch.float16, device=dev)
    q = torch.empty((args.batch, args.dim), dtype=torch.float16, device=dev)
    gen_rows(args.rows, args.dim, 1234, dev, latent=32, n_modes=4096, out=x, spread=0.7)
    gen_rows(args.batch, args.dim, 4321, dev, latent=32, n_modes=4096, out=q, spread=0.7)
    truth = exact_topk_fp64(x, q, 10)
    say("ground truth done")

    def build(compression):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        idx = cagra.build(cagra.IndexParams(graph_degree=args.degree, intermediate_graph_degree=2 * args.degree,
                                            compression=compression), x, resources=res)
        res.sync()
        torch.cuda.synchronize()
        return idx, time.perf_counter() - t0

    def measure(index, algo):
        sp = cagra.SearchParams(itopk_size=args.itopk, algo=algo)
        nb = None
        for _ in range(args.warmup):
            _, nb = cagra.search(sp, index, q, 10, resources=res)
        res.sync()
        times = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, nb = cagra.search(sp, index, q, 10, resources=res)
            res.sync()
            times.append((time.perf_counter() - t0) * 1e3)
        ids = nb.cpu().numpy().view("uint32").astype("int64")
        recall = sum(len(set(a) & set(b)) for a, b in zip(ids, truth)) / truth.size
        return {"ms_median": round(statistics.median(times), 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3),
                "recall_at_10": round(recall, 4)}

    out = {"bench": "cagra_vpq", "rows": args.rows, "dim": args.dim, "batch": args.batch, "graph_degree": args.degree,
           "itopk": args.itopk, "device": torch.cuda.get_device_name(0), "row_bytes_fp16": 2 * args.dim, "cases": []}
    _, warm = build(None)  # the first build of a process pays the one-time costs
    plain, t_plain = build(None)
    out["build_s_uncompressed"] = round(t_plain, 3)
    del plain
    say(f"uncompressed build {t_plain:.2f} s (first build of the process {warm:.2f} s)")
    for pq_len in args.pq_lens:
        comp = cagra.CompressionParams(pq_dim=args.dim // pq_len)
        cidx, t_comp = build(comp)
        vq_n, pq_n, got_len, row_len, dim = cidx._vpq_info()
        assert (got_len, dim) == (pq_len, args.dim) and row_len == 4 * (1 + -(-(args.dim // pq_len) // 4))
        case = {"pq_len": pq_len, "vq_n_centers": vq_n, "row_len": row_len, "build_s": round(t_comp, 3),
                "build_s_added_by_compression": round(t_comp - t_plain, 3),
                "dataset_bytes": args.rows * row_len + 2 * (vq_n * dim + pq_n * pq_len),
                "dataset_bytes_uncompressed": args.rows * args.dim * 2}
        twin = cagra.from_graph(cidx.graph, x, resources=res)  # the same graph over the original rows
        for algo in ("single_cta", "multi_cta"):
            case[algo] = {"compressed": measure(cidx, algo), "uncompressed_same_graph": measure(twin, algo)}
            say(pq_len, algo, case[algo])
        out["cases"].append(case)
        del cidx, twin
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

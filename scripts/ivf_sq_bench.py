"""IVF-SQ at the C2 shape (10M x 128 fp32 rows, n_lists 4096, n_probes 64, 10k queries, k 10): build time, ms per search,
recall@10 against exact search, and - alternating with it, on the same rows - the IVF-Flat search on its scan kernel alone
(CUVS_AMD_DEBUG_SWITCHES=1 CUVS_AMD_FLAT_SCAN3=0: set this in the environment; the flat index is searched through a handle
created under it). Prints one JSON line.

  python scripts/ivf_sq_bench.py [--rows N] [--reps R] [--skip-flat]
  (kernel time: rocprofv3 --kernel-trace --stats -- python scripts/ivf_sq_bench.py --reps 3 --skip-flat)"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--n-lists", type=int, default=4096)
    ap.add_argument("--n-probes", type=int, default=64)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-flat", action="store_true")
    a = ap.parse_args()
    from cuvs_amd.common import Resources
    from cuvs_amd.neighbors import brute_force, ivf_flat, ivf_sq

    res = Resources()
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    # clustered rows: 4096 blob centres + noise (uniform rows make every IVF index look the same)
    cent = torch.rand((a.n_lists, a.dim), generator=g, device="cuda")
    lab = torch.randint(0, a.n_lists, (a.rows,), generator=g, device="cuda")
    x = cent[lab] + 0.15 * torch.randn((a.rows, a.dim), generator=g, device="cuda")
    del lab
    q = cent[torch.randint(0, a.n_lists, (a.queries,), generator=g, device="cuda")] + 0.15 * torch.randn(
        (a.queries, a.dim), generator=g, device="cuda")
    out = {"shape": f"{a.rows}x{a.dim} f32, n_lists {a.n_lists}, n_probes {a.n_probes}, {a.queries} queries, k {a.k}"}

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            res.sync()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        return ts[len(ts) // 2]

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sq = ivf_sq.build(ivf_sq.IndexParams(n_lists=a.n_lists, kmeans_n_iters=20, max_train_points_per_cluster=256), x, resources=res)
    res.sync()
    out["sq_build_s"] = round(time.perf_counter() - t0, 3)
    sp = ivf_sq.SearchParams(n_probes=a.n_probes)
    flat = None
    if not a.skip_flat:
        t0 = time.perf_counter()
        flat = ivf_flat.build(ivf_flat.IndexParams(n_lists=a.n_lists, kmeans_n_iters=20), x, resources=res)
        res.sync()
        out["flat_build_s"] = round(time.perf_counter() - t0, 3)
        fres = Resources()  # created under the environment's switches (CUVS_AMD_FLAT_SCAN3=0)
        fp = ivf_flat.SearchParams(n_probes=a.n_probes)
    sq_ms, flat_ms = [], []
    for _ in range(a.reps):  # alternating: the two searches see the same machine state
        sq_ms.append(timed(lambda: ivf_sq.search(sp, sq, q, a.k, resources=res), 1))
        if flat is not None:
            flat_ms.append(timed(lambda: ivf_flat.search(fp, flat, q, a.k, resources=fres), 1))
    out["sq_search_ms"] = round(sorted(sq_ms)[len(sq_ms) // 2], 3)
    if flat_ms:
        out["flat_scan_kernel_search_ms"] = round(sorted(flat_ms)[len(flat_ms) // 2], 3)
        out["flat_scan3"] = os.environ.get("CUVS_AMD_FLAT_SCAN3", "1")
    _, si = ivf_sq.search(sp, sq, q, a.k, resources=res)
    bf = brute_force.build(x, resources=res)
    _, ti = brute_force.search(bf, q, a.k, resources=res)
    res.sync()
    si, ti = si.cpu(), ti.cpu()
    hits = sum(len(set(si[r].tolist()) & set(ti[r].tolist())) for r in range(a.queries))
    out["sq_recall_at_k"] = round(hits / (a.queries * a.k), 4)
    if flat is not None:
        _, fi = ivf_flat.search(fp, flat, q, a.k, resources=fres)
        res.sync()
        fi = fi.cpu()
        out["flat_recall_at_k"] = round(sum(len(set(fi[r].tolist()) & set(ti[r].tolist())) for r in range(a.queries)) / (a.queries * a.k), 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

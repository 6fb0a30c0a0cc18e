"""Times cuvsVamanaBuild at the defaults on rows ~ N(0.1, 2.0) and prints one JSON line: the median wall time of --reps builds
after one warm-up (device synchronised before and after each), the per-phase split of one more build (the library's profile
hooks: HIP events around the search, the forward prune, the reverse sort and the reverse prune of every batch), the graph's
edge count, and recall@10 of the graph through a CAGRA search (invalid slots replaced by node 0, itopk 64 and 512) against the exact
brute-force neighbours. With --cagra it also times cuvsCagraBuild (graph degree 32) on the same rows, for orientation.

    python scripts/bench_vamana.py [--rows 1000000] [--dim 128] [--reps 5] [--cagra] [--lib other/libcuvs_c.so]

--lib loads another build of the library (a before / after comparison of one change)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuvs_amd._lib as _lib  # noqa: E402

PHASES = ("vamana_search", "vamana_prune", "vamana_reverse_sort", "vamana_reverse_prune")


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def timed_builds(fn, reps, budget_s):
    """One warm-up, then up to `reps` timed calls (fewer when the warm-up shows they would not fit `budget_s`)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    keep = fn()
    torch.cuda.synchronize()
    warm = time.perf_counter() - t0
    say(f"  warm-up {warm:.3f} s")
    reps = max(1, min(reps, int(budget_s / max(warm, 1e-3))))
    times = []
    for _ in range(reps):
        del keep
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keep = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        say(f"  run {times[-1]:.3f} s")
    return keep, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--budget-s", type=float, default=240.0, help="wall time the timed builds of one builder may take")
    ap.add_argument("--cagra", action="store_true")
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    from cuvs_amd.common import Resources
    from cuvs_amd.neighbors import brute_force, cagra, vamana

    lib = _lib.lib()
    res = Resources()
    gen = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.randn((args.rows, args.dim), generator=gen, device="cuda") * 2.0 + 0.1
    q = torch.randn((args.queries, args.dim), generator=gen, device="cuda") * 2.0 + 0.1
    _, truth = brute_force.search(brute_force.build(x, resources=res), q, 10, resources=res)
    res.sync()
    truth = truth.cpu().numpy().astype("int64")

    def recall_of(index):
        out = {}
        for itopk in (64, 512):
            _, nb = cagra.search(cagra.SearchParams(itopk_size=itopk), index, q, 10, resources=res)
            res.sync()
            nb = nb.cpu().numpy().astype("int64")
            out[f"itopk_{itopk}"] = round(sum(len(set(a) & set(b)) for a, b in zip(nb, truth)) / truth.size, 4)
        return out

    out = {"bench": "vamana_build", "rows": args.rows, "dim": args.dim, "device": torch.cuda.get_device_name(0),
           "lib": args.lib or "in-tree"}
    params = vamana.IndexParams()
    say("vamana build")
    idx, times = timed_builds(lambda: vamana.build(params, x, resources=res), args.reps, args.budget_s)
    out["vamana_build_s"] = {"median": round(statistics.median(times), 4), "runs": [round(t, 4) for t in times]}
    del idx
    lib.cuvsAmdProfileEnable(1)
    idx = vamana.build(params, x, resources=res)
    torch.cuda.synchronize()
    lib.cuvsAmdProfileEnable(0)
    out["phases_ms"] = {}
    for name in PHASES:
        ms = C.c_double(0)
        n = lib.cuvsAmdProfileCollect(name.encode(), C.byref(ms))
        out["phases_ms"][name] = {"total": round(ms.value, 2), "batches": n}
    g = idx.graph
    out["medoid"] = idx.medoid
    out["edges_per_node"] = round(float((g != -1).sum().item()) / args.rows, 3)
    g0 = torch.where(g == -1, torch.zeros_like(g), g)
    out["vamana_recall_at_10_through_cagra"] = recall_of(cagra.from_graph(g0, x, resources=res))
    del idx, g, g0
    if args.cagra:
        say("cagra build")
        cp = cagra.IndexParams(graph_degree=32, intermediate_graph_degree=64)
        cidx, times = timed_builds(lambda: cagra.build(cp, x, resources=res), args.reps, args.budget_s)
        out["cagra_build_s"] = {"median": round(statistics.median(times), 4), "runs": [round(t, 4) for t in times]}
        out["cagra_recall_at_10"] = recall_of(cidx)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

"""Queries/s and recall@10 of the ScaNN search: 1M x 128 random blobs, 1000 leaves, 10k queries of the same blobs.

    python scripts/bench_scann_search.py [--rows 1000000] [--dim 128] [--leaves 1000] [--queries 10000] [--out FILE.json]

For pq_bits 4 and 8, n_reorder 0 and 100 and a few n_probes: the median wall time of `--steps` searches between two
synchronisations after `--warmup` calls (the first of which builds the search-side lists), recall@10 against exact brute force, the
(entry, query) pairs the scan scored, and the scan kernel's own time by the library's event timing in a run of its own. The scan's
FLOP rate counts pairs x 2 x dim against the 2517 TFLOP/s dense bf16 matrix peak of one MI355X."""
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
from cuvs_amd.common import Resources  # noqa: E402
from cuvs_amd.neighbors import brute_force, scann  # noqa: E402
from scripts.bench_scann import blobs  # noqa: E402

PEAK_BF16_TFLOPS = 2516.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--leaves", type=int, default=1000)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--probes", type=int, nargs="+", default=[5, 20, 50])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = Resources()
    both = blobs(a.rows + a.queries, a.dim, 0)
    x, q = both[:a.rows].contiguous(), both[a.rows:].contiguous()
    del both
    _, truth = brute_force.search(brute_force.build(x), q, 10)
    torch.cuda.synchronize()
    out = {"rows": a.rows, "dim": a.dim, "n_leaves": a.leaves, "queries": a.queries, "device": torch.cuda.get_device_name(0),
           "steps": a.steps, "warmup": a.warmup, "runs": []}
    for bits in (4, 8):
        idx = scann.build(scann.IndexParams(n_leaves=a.leaves, pq_bits=bits, reordering_bf16=True), x, resources=res)
        for n_reorder in (0, 100):
            for n_probes in a.probes:
                sp = scann.SearchParams(n_probes=n_probes, n_reorder=n_reorder)
                run = lambda: scann.search(sp, idx, q, 10, resources=res)  # noqa: E731
                for _ in range(a.warmup):
                    run()
                torch.cuda.synchronize()
                times = []
                for _ in range(a.steps):
                    t0 = time.perf_counter()
                    _, nb = run()
                    torch.cuda.synchronize()
                    times.append(time.perf_counter() - t0)
                stats = scann.search_last_stats()
                hit = (nb[:, :, None] == truth[:, None, :]).any(2).float().sum(1).mean().item() / 10
                ms = C.c_double(0)
                lib().cuvsAmdProfileCollect(b"scann_scan_kernel", None)
                lib().cuvsAmdProfileEnable(1)
                run()
                torch.cuda.synchronize()
                lib().cuvsAmdProfileEnable(0)
                launches = lib().cuvsAmdProfileCollect(b"scann_scan_kernel", C.byref(ms))
                t = statistics.median(times)
                tflops = stats[1] * 2.0 * a.dim / (ms.value / 1e3) / 1e12
                r = {"pq_bits": bits, "n_reorder": n_reorder, "n_probes": n_probes, "median_s": t, "min_s": min(times), "max_s": max(times),
                     "queries_per_s": a.queries / t, "recall_at_10": hit, "units": stats[0], "pairs": stats[1], "units_book_from_global": stats[2],
                     "duplicates_dropped": stats[3], "scan_kernel_s": ms.value / 1e3, "scan_kernel_launches": launches,
                     "scan_tflops": tflops, "scan_share_of_bf16_peak": tflops / PEAK_BF16_TFLOPS}
                out["runs"].append(r)
                print("bits %d reorder %3d probes %3d: %9.0f q/s  recall@10 %.4f  scan %.2f ms = %.1f TFLOP/s (%.1f %% of peak)" %
                      (bits, n_reorder, n_probes, r["queries_per_s"], hit, ms.value, tflops, 100 * r["scan_share_of_bf16_peak"]), flush=True)
        del idx
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

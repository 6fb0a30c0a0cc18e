#!/usr/bin/env python3
"""Tail phase of a tiered search, both paths against the composition a caller would otherwise write.

One IVF-Flat ANN tier over --ann-rows x 128 rows; per tail size in {1, 1k, 10k, 100k} the tier is extended by that many rows and
searched with batches of {1, 10, 64, 1000, 10000} queries, k = 10. Per cell, in one process, alternating:

  ann       the same ANN search alone (a standalone IVF-Flat index built with the same parameters: the build is deterministic)
  fused     cuvsTieredIndexSearch on a handle made with CUVS_AMD_TIERED_PATH=fused     (the single-launch kernel; batches <= 64)
  composed  cuvsTieredIndexSearch on a handle made with CUVS_AMD_TIERED_PATH=composed  (threshold append + merge kernel)
  default   cuvsTieredIndexSearch on a plain handle (the library's choice)
  baseline  cuvsBruteForceSearch on the tail rows (cuvsBruteForceBuild once per tail size, not timed), the ANN search, device ->
            host copies, a host merge

The tail phase of a path is its time minus `ann`. Times are host clocks around calls that end in a stream synchronise, the
median of --reps rounds after --warmup rounds; the three tiered results must agree bit for bit before anything is timed.
Writes one JSON document (--out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAILS = [1, 1000, 10000, 100000]
BATCHES = [1, 10, 64, 1000, 10000]
DIM, K = 128, 10


def switched_resources(value):
    """A handle whose tail phase is pinned to one path (the switches are read when a handle is created)."""
    import cuvs_amd

    old = {n: os.environ.get(n) for n in ("CUVS_AMD_DEBUG_SWITCHES", "CUVS_AMD_TIERED_PATH")}
    os.environ["CUVS_AMD_DEBUG_SWITCHES"] = "1"
    os.environ["CUVS_AMD_TIERED_PATH"] = value
    try:
        return cuvs_amd.common.Resources()
    finally:
        for n, v in old.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v


def host_merge(ad, ai, bd, bi, ann_rows, k):
    """What a caller of the three library calls does on the host: shift the tail ids, order the union by (distance, id)."""
    d = np.concatenate([ad, bd], axis=1)
    big = np.iinfo(np.int64).max
    missing = (ai < 0) | (ai >= ann_rows)  # a slot the ANN tier could not fill
    d[:, : ad.shape[1]][missing] = np.finfo(np.float32).max
    i = np.concatenate([np.where(missing, big, ai), np.where(bi < 0, big, bi + ann_rows)], axis=1)
    order = np.lexsort((i, d), axis=1)[:, :k]
    return np.take_along_axis(d, order, 1), np.take_along_axis(i, order, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ann-rows", type=int, default=200000)
    ap.add_argument("--n-lists", type=int, default=512)
    ap.add_argument("--n-probes", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--tails", type=int, nargs="*", default=TAILS)
    ap.add_argument("--batches", type=int, nargs="*", default=BATCHES)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiered_tail_bench.json"))
    args = ap.parse_args()

    import torch

    import cuvs_amd
    from cuvs_amd.neighbors import brute_force, ivf_flat, tiered_index as T

    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    res = {"default": cuvs_amd.common.Resources(), "fused": switched_resources("fused"), "composed": switched_resources("composed")}
    rng = np.random.default_rng(0)
    # clustered rows, so that the ANN tier is a healthy one: its k-th distance is a bound almost no tail row beats
    centers = rng.normal(0, 4, size=(256, DIM)).astype(np.float32)

    def draw(n):
        return (centers[rng.integers(0, len(centers), n)] + rng.normal(0, 1, size=(n, DIM))).astype(np.float32)

    base = torch.from_numpy(draw(args.ann_rows)).cuda()
    queries = torch.from_numpy(draw(max(args.batches))).cuda()
    up = ivf_flat.IndexParams(n_lists=args.n_lists, kmeans_n_iters=10)
    sp = ivf_flat.SearchParams(n_probes=args.n_probes)
    params = T.IndexParams(algo="ivf_flat", upstream_params=up, min_ann_rows=args.ann_rows // 2)
    ann_alone = ivf_flat.build(up, base, resources=res["default"])
    cells = []
    idx = T.build(params, base, resources=res["default"])
    all_tail = torch.from_numpy(draw(max(args.tails))).cuda()
    have = 0
    for tail in sorted(args.tails):
        T.extend(idx, all_tail[have:tail], resources=res["default"])  # the tail grows to the next size
        have = tail
        rows = all_tail[:tail]
        assert T.info(idx)[:2] == (args.ann_rows + tail, args.ann_rows)
        bf = brute_force.build(rows, resources=res["default"])  # (outside the timed calls: a caller keeps it between searches)
        for m in args.batches:
            q = queries[:m].contiguous()
            nb = torch.empty((m, K), dtype=torch.int64, device="cuda")
            ds = torch.empty((m, K), dtype=torch.float32, device="cuda")

            def tiered(which):
                return lambda: T.search(sp, idx, q, K, neighbors=nb, distances=ds, resources=res[which])

            def ann():
                return ivf_flat.search(sp, ann_alone, q, K, neighbors=nb, distances=ds, resources=res["default"])

            def baseline():
                bd, bi = brute_force.search(bf, q, K, resources=res["default"])
                ad, ai = ivf_flat.search(sp, ann_alone, q, K, resources=res["default"])
                return host_merge(ad.cpu().numpy(), ai.cpu().numpy(), bd.cpu().numpy(), bi.cpu().numpy(), args.ann_rows, K)

            runs = {"ann": ann, "composed": tiered("composed"), "default": tiered("default"), "baseline": baseline}
            if m <= 64:
                runs["fused"] = tiered("fused")
            # the paths agree bit for bit, and with the host composition (ids; the ANN tier may return fewer than k rows)
            got = {}
            for name in ("composed", "default", "fused"):
                if name in runs:
                    d, i = runs[name]()
                    got[name] = (d.cpu().numpy().view(np.uint32).copy(), i.cpu().numpy().copy())
            for name in got:
                assert (got[name][0] == got["composed"][0]).all() and (got[name][1] == got["composed"][1]).all(), name
            hd, hi = baseline()
            assert (hi == got["composed"][1]).all() and (hd.view(np.uint32) == got["composed"][0]).all(), "host composition"
            before = T.counters()
            times = {name: [] for name in runs}
            for rep in range(args.warmup + args.reps):
                for name, fn in runs.items():  # alternating: every path sees the same neighbours on the machine
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()  # (the calls synchronise the handle's stream before they return)
                    torch.cuda.synchronize()
                    if rep >= args.warmup:
                        times[name].append((time.perf_counter() - t0) * 1e6)
            after = T.counters()
            med = {name: statistics.median(v) for name, v in times.items()}
            cell = {"tail": tail, "batch": m, "median_us": {n: round(v, 1) for n, v in med.items()},
                    "min_us": {n: round(min(v), 1) for n, v in times.items()},
                    "tail_phase_us": {n: round(med[n] - med["ann"], 1) for n in med if n != "ann"},
                    "exact_redos": after[2] - before[2]}
            cells.append(cell)
            print(json.dumps(cell), flush=True)
    doc = {"what": "tail phase of a tiered search = tiered search - the same ANN search alone; microseconds, host clock around "
                   "synchronised calls, median of reps",
           "dim": DIM, "k": K, "ann": {"algo": "ivf_flat", "rows": args.ann_rows, "n_lists": args.n_lists, "n_probes": args.n_probes},
           "warmup": args.warmup, "reps": args.reps, "device": torch.cuda.get_device_name(0), "cells": cells}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

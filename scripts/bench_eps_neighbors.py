"""Epsilon neighbourhood at 100k x 100k: dense, degrees-only and the two-call CSR form of
cuvs_amd.neighbors.epsilon_neighborhood, next to the composition a caller had before it: pairwise_distance(l2_unexpanded)
into fp32 row slabs, `<= eps` and nonzero in torch.

HIP events around each call, 2 warm-up calls, the median of --reps (>= 10) timed ones. Every time is also given as a
multiple of the VALU floor: 2 m n dim lane-operations (one subtraction and one fma per pair element) at the packed fp32
rate of the device, 256 CUs x 4 SIMDs x 32 lane-operations per clock x 2.4 GHz = 78.6e12 per second (the tile kernel
issues v_pk_add_f32 / v_pk_fma_f32).

    python scripts/bench_eps_neighbors.py [--rows 100000] [--dims 16,128] [--reps 10] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cuvs_amd.common import Resources  # noqa: E402
from cuvs_amd.distance import pairwise_distance  # noqa: E402
from cuvs_amd.neighbors import epsilon_neighborhood as E  # noqa: E402

PACKED_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9


def blobs(rows, dim, per_center, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    centers = torch.rand(rows // per_center, dim, device="cuda", generator=g) * 20 - 10
    labels = torch.randperm(rows, device="cuda", generator=g) % (rows // per_center)
    return (centers[labels] + 0.01 * torch.randn(rows, dim, device="cuda", generator=g)).contiguous()


def timed(fn, res, reps):
    for _ in range(2):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--dims", default="16,128")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--slab", type=int, default=5000, help="rows per slab of the composed baseline (5000 x 100k fp32 = 2 GB)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = Resources()
    eps = 4.0  # radius 2, squared
    results = []
    for dim in [int(d) for d in args.dims.split(",")]:
        n = args.rows
        x = blobs(n, dim, 100, dim)
        floor_ms = 2.0 * n * n * dim / PACKED_LANE_OPS_PER_S * 1e3
        adj = torch.empty((n, n), dtype=torch.bool, device="cuda")
        vd = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        indptr = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        E.compute(x, x, eps, adj=False, vd=vd, resources=res)
        res.sync()
        edges = int(vd[n])
        indices = torch.empty(edges, dtype=torch.int64, device="cuda")

        def csr_two_calls():
            E.csr_count(x, x, eps, indptr=indptr, resources=res)
            E.csr_fill(x, x, eps, indptr, indices, resources=res)

        def csr_one_call():
            E.csr_fill(x, x, eps, indptr, indices_cap, max_k=cap, resources=res)

        cap = int(vd[:n].max())
        indices_cap = torch.empty(n * cap, dtype=torch.int64, device="cuda")
        tile = torch.empty((min(args.slab, n), n), dtype=torch.float32, device="cuda")
        found = [0]

        def composed():
            total = 0
            for r0 in range(0, n, args.slab):
                rows = min(args.slab, n - r0)
                d = pairwise_distance(x[r0:r0 + rows], x, out=tile[:rows], metric="l2_unexpanded", resources=res)
                total += (d <= eps).nonzero().shape[0]
            found[0] = total

        runs = [("dense", lambda: E.compute(x, x, eps, adj=adj, vd=vd, resources=res)),
                ("degrees_only", lambda: E.compute(x, x, eps, adj=False, vd=vd, resources=res)),
                ("csr_two_calls", csr_two_calls),
                ("csr_one_call_max_k", csr_one_call),
                ("composed_pairwise_le_nonzero", composed)]
        for name, fn in runs:
            med, lo, hi = timed(fn, res, args.reps)
            row = dict(shape=f"{n}x{n}x{dim}", form=name, median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3),
                       valu_floor_ms=round(floor_ms, 3), times_floor=round(med / floor_ms, 2), edges=edges, reps=args.reps)
            if name == "composed_pairwise_le_nonzero":
                row["edges_composed"] = found[0]
            results.append(row)
            print(json.dumps(row), flush=True)
        del adj, tile, indices, indices_cap
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(rate="packed fp32: 78.6e12 lane-operations per second", results=results), f, indent=1)


if __name__ == "__main__":
    main()

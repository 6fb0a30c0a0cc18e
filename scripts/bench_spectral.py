"""Timing of the spectral embedding: transform on n x dim rows, split into the kNN graph, the Laplacian and the
eigen-solver by the library's own stream events; for the eigen-solver the matrix-vector products, the time per Lanczos step and
the rate at which the re-orthogonalisation's algorithmic bytes (4 (j + 1) n 4 per step j) were moved. One JSON line on stdout.

    python scripts/bench_spectral.py [--n 100000 --dim 64 --k 15 --components 8 --steps 3 --warmup 1]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12        # bytes/s, the specification
HBM_ACHIEVABLE = 6.3e12  # bytes/s, what a streaming kernel reaches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--components", type=int, default=8)
    ap.add_argument("--clusters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ortho-n", type=int, default=4000000, help="columns of the re-orthogonalisation timed on its own (0: skip)")
    ap.add_argument("--ortho-j", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this timing needs the GPU"

    import cuvs_amd
    from cuvs_amd._lib import lib
    from cuvs_amd.preprocessing import spectral_embedding as se

    res = cuvs_amd.common.Resources()
    gen = torch.Generator(device="cuda").manual_seed(1)
    centres = torch.rand((args.clusters, args.dim), generator=gen, device="cuda") * 4.0
    x = centres[torch.arange(args.n, device="cuda") % args.clusters] + torch.randn((args.n, args.dim), generator=gen, device="cuda")
    x = x.contiguous()
    p = se.Params(n_components=args.components, n_neighbors=args.k, tolerance=1e-5, seed=0)

    for _ in range(args.warmup):
        se.transform(p, x, resources=res)
    torch.cuda.synchronize()
    lib().cuvsAmdProfileEnable(1)
    t = time.perf_counter()
    for _ in range(args.steps):
        se.transform(p, x, resources=res)
    torch.cuda.synchronize()
    total = (time.perf_counter() - t) / args.steps
    lib().cuvsAmdProfileEnable(0)
    parts = {}
    for name in ("sp_knn", "sp_symmetrise", "sp_laplacian", "sp_lanczos"):
        ms = C.c_double(0)
        lib().cuvsAmdProfileCollect(name.encode(), C.byref(ms))
        parts[name + "_ms"] = ms.value / args.steps
    stats = se.last_stats()
    m, k, n = int(stats["ncv"]), args.components, args.n
    # the steps of the solve: the first cycle takes j = 0 .. m - 1, every later one j = k .. m - 1
    js, left = [], int(stats["matvecs"])
    cycle = list(range(m))
    while left > 0:
        js += cycle[:left]
        left -= len(cycle)
        cycle = list(range(k, m))
    ortho_bytes = sum(4 * (j + 1) * n * 4 for j in js)
    solver_s = parts["sp_lanczos_ms"] * 1e-3
    out = dict(n=n, dim=args.dim, k=args.k, n_components=k, transform_ms=total * 1e3, **parts, **{key: int(v) for key, v in stats.items()},
               lanczos_step_us=solver_s / max(len(js), 1) * 1e6, ortho_algorithmic_gb=ortho_bytes / 1e9,
               ortho_bytes_rate_tbs=ortho_bytes / solver_s / 1e12 if solver_s else 0.0,
               share_of_hbm_peak=ortho_bytes / solver_s / HBM_PEAK if solver_s else 0.0,
               share_of_hbm_achievable=ortho_bytes / solver_s / HBM_ACHIEVABLE if solver_s else 0.0)
    if args.ortho_n:
        # the re-orthogonalisation on its own through its hook, at a size where the launches no longer dominate: the hook also
        # allocates, copies u once and reads the norm back, so this is a lower bound of the kernels' rate
        v = torch.randn((args.ortho_j, args.ortho_n), generator=gen, device="cuda") / args.ortho_n ** 0.5
        u = torch.randn(args.ortho_n, generator=gen, device="cuda")
        for _ in range(3):
            se.orthogonalize(v, u.clone(), resources=res)
        torch.cuda.synchronize()
        us = [u.clone() for _ in range(10)]
        torch.cuda.synchronize()
        t = time.perf_counter()
        for w in us:
            se.orthogonalize(v, w, resources=res)
        torch.cuda.synchronize()
        call = (time.perf_counter() - t) / len(us)
        nbytes = 4 * args.ortho_j * args.ortho_n * 4
        out.update(ortho_n=args.ortho_n, ortho_j=args.ortho_j, ortho_call_us=call * 1e6, ortho_call_tbs=nbytes / call / 1e12,
                   ortho_call_share_of_hbm_achievable=nbytes / call / HBM_ACHIEVABLE)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

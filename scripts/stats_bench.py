"""cuvs_amd.stats at 100k rows: the silhouette score at dim 16 and 128 with 10 and 1000 labels, the trustworthiness
score at 128 -> 2 with k = 5 and 15 for a good and a poor embedding, each next to

  * the VALU floor of 3.1t: 2 n^2 dim lane-operations at 78.6e12 per second,
  * the composition a user had before: cuvsPairwiseDistance into fp32 row slabs + torch index_add_ (silhouette), + a sort of
    every slab (trustworthiness) - the comparator a parent commit cannot be, since it has no such entry point,
  * the pair tile of 3.1t itself (epsilon_neighborhood.compute, degrees only) at the same shape: the silhouette tile is that tile
    with the fp64 epilogue in place of the bit-mask one, so 1 - eps / silhouette over the two tile kernels' own times
    (`tile_kernel_ms`, from the library's per-kernel HIP events in one more call) is the epilogue's share.

HIP events around each call, 2 warm-up calls, the median of 10 timed ones (1 and 3 for the compositions, which take seconds).
Every step runs in a process of its own under `timeout`; a step that fails or runs out of time is reported as such and the
others go on only if it ended by itself.

    python scripts/stats_bench.py [--rows 100000] [--out profiles/stats_bench.json] [--steps sil_16_10,trust_good_15,...]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_LANE_OPS_PER_S = 78.6e12
STEPS = (["sil_%d_%d" % (d, c) for d in (16, 128) for c in (10, 1000)] + ["silbase_%d_%d" % (d, c) for d in (16, 128) for c in (10, 1000)]
         + ["eps_16", "eps_128", "trust_good_5", "trust_good_15", "trust_poor_15", "trustbase_good_5", "trustbase_good_15"])


def timed(fn, reps, warm):
    import torch

    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return dict(median_ms=round(statistics.median(times), 3), min_ms=round(min(times), 3), max_ms=round(max(times), 3), reps=reps)


def kernel_ms(fn, name):
    """one more call with the library's per-kernel HIP events on: the time of the kernel `name` alone"""
    import ctypes as C

    import torch

    from cuvs_amd._lib import lib

    lib().cuvsAmdProfileCollect(name, None)
    lib().cuvsAmdProfileEnable(1)
    fn()
    torch.cuda.synchronize()
    lib().cuvsAmdProfileEnable(0)
    ms = C.c_double(0)
    lib().cuvsAmdProfileCollect(name, C.byref(ms))
    return round(ms.value, 3)


def blobs(n, dim, centers, seed):
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    c = torch.rand(centers, dim, device="cuda", generator=g) * 20 - 10
    y = torch.randint(0, centers, (n,), device="cuda", generator=g)
    return (c[y] + torch.randn(n, dim, device="cuda", generator=g)).contiguous(), y.to(torch.int32)


def embedding(n, good, seed):
    """X [n, 128] near a 2-D sheet; E its two coordinates (good) or random (poor)"""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    z = torch.randn(n, 2, device="cuda", generator=g)
    x = (z @ torch.randn(2, 128, device="cuda", generator=g) + 0.01 * torch.randn(n, 128, device="cuda", generator=g)).contiguous()
    e = z.contiguous() if good else torch.randn(n, 2, device="cuda", generator=g)
    return x, e


def silhouette_composition(X, y, n_labels, res, out_slab):
    import torch

    from cuvs_amd.distance import pairwise_distance

    n = X.shape[0]
    yl = y.long()
    cnt = torch.bincount(yl, minlength=n_labels).float()
    scores = torch.empty(n, dtype=torch.float32, device="cuda")
    slab = out_slab.shape[0]
    for r0 in range(0, n, slab):
        r1 = min(n, r0 + slab)
        D = out_slab[:r1 - r0]
        pairwise_distance(X[r0:r1], X, out=D, metric="sqeuclidean", resources=res)
        res.sync()
        S = torch.zeros((r1 - r0, n_labels), dtype=torch.float32, device="cuda").index_add_(1, yl, D)
        rows = torch.arange(r1 - r0, device="cuda")
        own = yl[r0:r1]
        a = S[rows, own] / (cnt[own] - 1)
        S = S / cnt
        S[rows, own] = float("inf")
        b = S.min(dim=1).values
        s = (b - a) / torch.maximum(a, b)
        s[cnt[own] == 1] = 0
        scores[r0:r1] = s
    return scores.double().mean().item()


def trustworthiness_composition(X, E, k, res, out_slab):
    import torch

    from cuvs_amd.distance import pairwise_distance
    from cuvs_amd.neighbors import brute_force

    n = X.shape[0]
    _, nb = brute_force.search(brute_force.build(E), E, k + 1)
    nb = nb[:, 1:]  # (the row itself comes first but for duplicates)
    slab = out_slab.shape[0]
    cols = torch.arange(n, device="cuda")
    t = 0
    for r0 in range(0, n, slab):
        r1 = min(n, r0 + slab)
        D = out_slab[:r1 - r0]
        pairwise_distance(X[r0:r1], X, out=D, metric="sqeuclidean", resources=res)
        res.sync()
        rows = torch.arange(r1 - r0, device="cuda")
        D[rows, r0 + rows] = -1.0  # the row itself at place 0: the others are ranked from 1
        order = D.argsort(dim=1)
        rank = torch.empty_like(order).scatter_(1, order, cols.expand(r1 - r0, n))
        t += int((rank.gather(1, nb[r0:r1]) - k).clamp_(min=0).sum().item())
    return 1.0 - t * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))


def run_step(step, n):
    import torch

    from cuvs_amd import stats
    from cuvs_amd.common import Resources
    from cuvs_amd.neighbors import epsilon_neighborhood

    res = Resources()
    kind, *rest = step.split("_")
    out = dict(step=step, rows=n)
    if kind in ("sil", "silbase"):
        dim, n_labels = int(rest[0]), int(rest[1])
        X, y = blobs(n, dim, n_labels, dim + n_labels)
        out.update(dim=dim, labels=n_labels, floor_ms=round(2.0 * n * n * dim / VALU_LANE_OPS_PER_S * 1e3, 3))
        if kind == "sil":
            out.update(timed(lambda: stats.silhouette_score(X, y, n_labels, resources=res), 10, 2))
            out["score"] = stats.silhouette_score(X, y, n_labels, resources=res)
            out["tile_kernel_ms"] = kernel_ms(lambda: stats.silhouette_score(X, y, n_labels, resources=res), b"sil_tile_kernel")
            st = stats.last_stats()
            out.update(tiles=st["tiles"], slabs=st["slabs"], straddling_tiles=st["straddling_or_passed"])
        else:
            slab = torch.empty(((1 << 30) // (4 * n), n), dtype=torch.float32, device="cuda")
            out.update(timed(lambda: silhouette_composition(X, y, n_labels, res, slab), 3, 1))
            out["score"] = silhouette_composition(X, y, n_labels, res, slab)
    elif kind == "eps":
        dim = int(rest[0])
        X, _ = blobs(n, dim, 10, dim + 10)
        out.update(dim=dim, floor_ms=round(2.0 * n * n * dim / VALU_LANE_OPS_PER_S * 1e3, 3))
        out.update(timed(lambda: epsilon_neighborhood.compute(X, X, 1.0, adj=False, resources=res), 10, 2))
        out["tile_kernel_ms"] = kernel_ms(lambda: epsilon_neighborhood.compute(X, X, 1.0, adj=False, resources=res), b"eps_tile_kernel_dense")
    else:
        good, k = rest[0] == "good", int(rest[1])
        X, E = embedding(n, good, k)
        out.update(dim=128, dim_embedded=2, k=k, embedding=rest[0], floor_ms=round(2.0 * n * n * 128 / VALU_LANE_OPS_PER_S * 1e3, 3))
        if kind == "trust":
            out.update(timed(lambda: stats.trustworthiness_score(X, E, n_neighbors=k, resources=res), 10, 2))
            out["score"] = stats.trustworthiness_score(X, E, n_neighbors=k, resources=res)
            out["pairs_past_the_screen"] = stats.last_stats()["straddling_or_passed"]
            out["tile_kernel_ms"] = kernel_ms(lambda: stats.trustworthiness_score(X, E, n_neighbors=k, resources=res), b"rank_tile_kernel")
            out["share_of_pairs_past_the_screen"] = round(out["pairs_past_the_screen"] / (n * (n - 1.0)), 6)
        else:
            slab = torch.empty((1024, n), dtype=torch.float32, device="cuda")
            out.update(timed(lambda: trustworthiness_composition(X, E, k, res, slab), 3, 1))
            out["score"] = trustworthiness_composition(X, E, k, res, slab)
    out["x_floor"] = round(out["median_ms"] / out["floor_ms"], 2)
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stats_bench.json"))
    ap.add_argument("--steps", default=",".join(STEPS))
    ap.add_argument("--step", default=None, help="run one step in this process (used by the driver)")
    ap.add_argument("--step-timeout", type=int, default=150)
    args = ap.parse_args()
    if args.step is not None:
        run_step(args.step, args.rows)
        return 0
    results = []
    for step in args.steps.split(","):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--rows", str(args.rows)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        lines = [line[7:] for line in p.stdout.splitlines() if line.startswith("RESULT ")]
        if p.returncode == 0 and lines:
            results.append(json.loads(lines[-1]))
            print(lines[-1], flush=True)
        else:
            results.append(dict(step=step, rows=args.rows, failed=True, returncode=p.returncode, stderr=p.stderr[-400:]))
            print("step %s failed with status %d: %s" % (step, p.returncode, p.stderr[-400:]), flush=True)
        with open(args.out, "w") as f:
            json.dump(dict(valu_lane_ops_per_s=VALU_LANE_OPS_PER_S, results=results), f, indent=1)
        if p.returncode not in (0, 1, 2):  # a time limit, an abort or a fault: nothing more is started on the device
            print("stopping after step %s" % step, flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Times cuvs_amd.distance.masked_l2_nn and cross_component_nn on the GPU and writes one JSON file.

masked_l2_nn: m = n = 100k, dim 64, 1000 groups of 100 rows, adj at densities 1.0 / 0.1 / 0.01, drawn per (row, group) ("iid") and
per (128-row block, group) ("blocked": the rows of a tile share their mask, so switched-off tiles exist). Beside each time: the
share of 128 x 128 pair tiles computed. Baselines: the composition on the parent commit (pairwise_distance in row batches, a
torch mask, argmin), and the unmasked cuvsAmdFusedArgmin at the same shape as the ceiling for density 1.0.
cross_component_nn: n = 1M, dim 16, about 1000 compact components; baseline: the same composition on every eighth row, scaled.
Times are medians of `--reps` calls after one warm-up, host clock around a device synchronise."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cuvs_amd import common, distance  # noqa: E402
from cuvs_amd._lib import check, lib  # noqa: E402


def timed(f, reps):
    f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(ms_median=statistics.median(ts), ms_min=min(ts), ms_max=max(ts), reps=reps)


def composed(res, x, y, allowed_of_rows, batch, rows=None):
    """pairwise_distance in row batches + mask + argmin; allowed_of_rows(r0, r1) -> bool [r1 - r0, n]"""
    rows = range(0, x.shape[0], batch) if rows is None else rows
    out_i, out_d = [], []
    for r0 in rows:
        r1 = min(r0 + batch, x.shape[0])
        d = distance.pairwise_distance(x[r0:r1], y, metric="sqeuclidean", resources=res)
        d.masked_fill_(~allowed_of_rows(r0, r1), float("inf"))
        v, i = d.min(1)
        out_i.append(i)
        out_d.append(v)
    return torch.cat(out_i), torch.cat(out_d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/masked_nn_bench.json")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--cc-n", type=int, default=1_000_000)
    a = ap.parse_args()
    res = common.Resources()
    g = torch.Generator(device="cuda").manual_seed(0)
    out = dict(device=torch.cuda.get_device_name(0), masked=[], cross_component={})

    # ---- masked_l2_nn
    n, dim, G = a.n, 64, 1000
    x = torch.randn(n, dim, device="cuda", generator=g)
    y = torch.randn(n, dim, device="cuda", generator=g)
    ends = (torch.arange(1, G + 1, device="cuda", dtype=torch.int64) * (n // G))
    group_of = torch.arange(n, device="cuda") // (n // G)
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    fused = timed(lambda: check(lib().cuvsAmdFusedArgmin(res.get_c_obj(), C.c_void_p(x.data_ptr()), C.c_int64(n), C.c_void_p(y.data_ptr()),
                                                         C.c_int64(n), C.c_int64(dim), C.c_void_p(labels.data_ptr()))), a.reps)
    out["fused_argmin_unmasked"] = dict(shape=[n, n, dim], **fused)
    for kind in ("iid", "blocked"):
        for density in (1.0, 0.1, 0.01):
            rows = n if kind == "iid" else -(-n // 128)
            adj = torch.rand(rows, G, device="cuda", generator=g) < density
            if kind == "blocked":
                adj = adj.repeat_interleave(128, 0)[:n].contiguous()
            t = timed(lambda: distance.masked_l2_nn(x, y, adj, ends, resources=res), a.reps)
            total, live = distance.masked_nn_last_stats(res)
            idx, dist = distance.masked_l2_nn(x, y, adj, ends, resources=res)
            base = timed(lambda: composed(res, x, y, lambda r0, r1: adj[r0:r1][:, group_of], 4096), max(1, a.reps // 2))
            bi, bd = composed(res, x, y, lambda r0, r1: adj[r0:r1][:, group_of], 4096)
            agree = float((idx == torch.where(torch.isinf(bd), -1, bi)).float().mean())
            out["masked"].append(dict(shape=[n, n, dim], groups=G, mask=kind, density=density, live_tile_share=live / total,
                                      masked_l2_nn=t, composed_pairwise_mask_argmin=base, ids_equal_to_composed=agree))
            print(out["masked"][-1], flush=True)

    # ---- cross_component_nn
    n, dim, k = a.cc_n, 16, 1000
    x = torch.randn(n, dim, device="cuda", generator=g)
    colors = torch.cat([torch.cdist(x[r:r + 65536], x[:k]).argmin(1) for r in range(0, n, 65536)]).to(torch.int32)
    t = timed(lambda: distance.cross_component_nn(x, colors, k, resources=res), max(1, a.reps // 2))
    total, live = distance.masked_nn_last_stats(res)
    every = 8
    batch = 1024
    base = timed(lambda: composed(res, x, x, lambda r0, r1: colors[r0:r1, None] != colors[None, :], batch, range(0, n, batch * every)), 1)
    out["cross_component"] = dict(shape=[n, dim], components=int(colors.unique().numel()), live_tile_share=live / total, cross_component_nn=t,
                                  composed_on_every_8th_row_batch=base, composed_scaled_ms=base["ms_median"] * every)
    print(out["cross_component"], flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

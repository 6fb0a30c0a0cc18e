"""Wall time of every stage of the ScaNN build: 1M x 128 random blobs, the default parameters, 1000 leaves.

    python scripts/bench_scann.py [--rows 1000000] [--dim 128] [--leaves 1000] [--out FILE.json]

The stages are run one by one through the public entry points, on device rows, each after a warm-up call and between two
synchronisations: the balanced fit on the 100000-row sample, the prediction of all rows, the AVQ centres at eta 1 and 2, the SOAR
labels, the PQ training on the residuals of the 100000-row sample, the encoding of the primary residuals (through the product
quantizer's own transform on materialised residuals: the build itself hands the centres to the encoder and writes no residuals),
the bf16 rows without and with noise shaping, and the whole build from device and from host rows. The SOAR kernel's FLOP rate counts
n_rows x n_leaves x dim x 2 multiply-adds against the 157 TFLOP/s fp32 matrix peak of one MI355X."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cuvs_amd._lib import lib  # noqa: E402
from cuvs_amd.cluster import kmeans  # noqa: E402
from cuvs_amd.common import Resources  # noqa: E402
from cuvs_amd.neighbors import scann  # noqa: E402
from cuvs_amd.preprocessing.quantize import pq  # noqa: E402

PEAK_TFLOPS = 157.3


def blobs(n, dim, seed, n_centers=1000, box=10.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    centers = (torch.rand((n_centers, dim), generator=g, device="cuda") * 2 - 1) * box
    pick = torch.randint(0, n_centers, (n,), generator=g, device="cuda")
    return (centers[pick] + torch.randn((n, dim), generator=g, device="cuda")).contiguous()


def timed(fn, warmup=1, reps=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    out = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--leaves", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = Resources()
    n, dim, L = a.rows, a.dim, a.leaves
    x = blobs(n, dim, 0)
    r = {"rows": n, "dim": dim, "n_leaves": L, "device": torch.cuda.get_device_name(0)}
    p = scann.IndexParams(n_leaves=L)
    m = min(p.kmeans_n_rows_train, n)
    sample = x[:: n // m][:m].contiguous()
    kp = kmeans.KMeansParams(n_clusters=L, hierarchical=True, hierarchical_n_iters=p.kmeans_n_iters)
    r["fit_s"], fit = timed(lambda: kmeans.fit(kp, sample, resources=res), warmup=0)
    centers = fit.centroids
    r["predict_s"], pred = timed(lambda: kmeans.predict(kp, x, centers, resources=res))
    labels = pred.labels
    for eta in (1.0, 2.0):
        r["avq_eta%g_s" % eta], c = timed(lambda: scann.avq_centers(x, labels, centers.clone(), eta, resources=res))
    avq = scann.avq_centers(x, labels, centers.clone(), 1.0, resources=res)
    r["soar_s"], soar = timed(lambda: scann.soar_labels(x, avq, labels, p.soar_lambda, resources=res), reps=3)
    flop = 2.0 * n * L * dim * 2
    r["soar_call_tflops"] = flop / r["soar_s"] / 1e12
    # the tile kernel alone, by the library's event timing (the call also computes the unit residuals and the centre norms)
    ms = C.c_double(0)
    lib().cuvsAmdProfileCollect(b"soar_tile_kernel", None)
    lib().cuvsAmdProfileEnable(1)
    scann.soar_labels(x, avq, labels, p.soar_lambda, resources=res)
    torch.cuda.synchronize()
    lib().cuvsAmdProfileEnable(0)
    r["soar_tile_kernel_launches"] = lib().cuvsAmdProfileCollect(b"soar_tile_kernel", C.byref(ms))
    r["soar_tile_kernel_s"] = ms.value / 1e3
    r["soar_tflops"] = flop / r["soar_tile_kernel_s"] / 1e12
    r["soar_share_of_fp32_peak"] = r["soar_tflops"] / PEAK_TFLOPS
    r["soar_same_leaf_share"] = float((soar == labels).float().mean())
    m2 = min(p.pq_n_rows_train, 100000, n)
    ids = torch.arange(m2, device="cuda") * (n // m2)
    resid = (x[ids] - avq[labels[ids].long()]).contiguous()
    qp = pq.QuantizerParams(pq_bits=p.pq_bits, pq_dim=dim // p.pq_dim, kmeans_n_iters=p.pq_train_iters,
                            max_train_points_per_pq_code=m2 // (1 << p.pq_bits))
    r["pq_train_s"], q = timed(lambda: pq.build(qp, resid, resources=res), warmup=0)
    all_resid = (x - avq[labels.long()]).contiguous()
    r["encode_primary_s"], _ = timed(lambda: pq.transform(q, all_resid, resources=res))
    del all_resid
    r["bf16_plain_s"], _ = timed(lambda: scann.quantize_bf16(x, resources=res))
    r["bf16_noise_shaping_s"], _ = timed(lambda: scann.quantize_bf16(x, 0.2 * float(x.norm(dim=1).mean()), resources=res))
    pb = scann.IndexParams(n_leaves=L, reordering_bf16=True)
    r["build_device_rows_s"], _ = timed(lambda: scann.build(pb, x, resources=res), warmup=0)
    xh = x.cpu().numpy()
    r["build_host_rows_s"], _ = timed(lambda: scann.build(pb, xh, resources=res), warmup=0)
    for k, v in r.items():
        print("%-28s %s" % (k, ("%.4f" % v) if isinstance(v, float) else v))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)
    assert np.isfinite(r["soar_tflops"])


if __name__ == "__main__":
    main()

"""Times cuvsPcaFit, cuvsPcaTransform and cuvsPcaInverseTransform at 1M x 768 -> 128 and 1M x 128 -> 32, column- and row-major, and
prints one JSON line. The covariance kernel is timed by the library's profile hook (HIP events around the launch); its share of
the fp32 matrix-core peak counts the 64 x 64 tile pairs it computes (the upper triangle, diagonal tiles whole).

    python scripts/bench_pca.py [--rows 1000000] [--reps 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuvs_amd._lib import lib  # noqa: E402
from cuvs_amd.common import Resources  # noqa: E402
from cuvs_amd.preprocessing import pca  # noqa: E402

FP32_MFMA_PEAK_TFLOPS = 157.3  # 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def kernel_ms(name, fn, reps):
    """Best of `reps` profiled calls (HIP events around the named launches of one call)."""
    best = float("inf")
    for _ in range(reps):
        lib().cuvsAmdProfileEnable(1)
        fn()
        torch.cuda.synchronize()
        lib().cuvsAmdProfileEnable(0)
        ms = C.c_double(0)
        n = lib().cuvsAmdProfileCollect(name, C.byref(ms))
        best = min(best, ms.value / max(n, 1))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    res = Resources()
    out = {"bench": "pca", "rows": args.rows, "device": torch.cuda.get_device_name(0), "cases": []}
    gen = torch.Generator(device="cuda").manual_seed(1)
    for d, k in ((768, 128), (128, 32)):
        base = torch.randn((args.rows, d), generator=gen, device="cuda") * torch.linspace(2.0, 0.1, d, device="cuda") + 1.0
        for layout in ("col_major", "row_major"):
            X = base if layout == "row_major" else base.t().contiguous().t()
            params = pca.Params(n_components=k)
            f = pca.fit(params, X, resources=res)
            t = pca.transform(params, X, f.components, f.singular_vals, f.mu, resources=res)
            fit_ms = timed(lambda: pca.fit(params, X, resources=res), args.reps)
            tr_ms = timed(lambda: pca.transform(params, X, f.components, f.singular_vals, f.mu, trans_input=t, resources=res), args.reps)
            y = torch.empty_like(X)
            inv_ms = timed(lambda: pca.inverse_transform(params, t, f.components, f.singular_vals, f.mu, output=y, resources=res),
                           args.reps)
            cov_ms = kernel_ms(b"pca_cov_kernel", lambda: pca.fit(params, X, resources=res), args.reps)
            jac_ms = kernel_ms(b"pca_jacobi", lambda: pca.fit(params, X, resources=res), args.reps)
            sweeps = C.c_int(0)
            lib().cuvsAmdPcaLastSweeps(C.byref(sweeps))
            tiles = (d + 63) // 64
            flop = 2.0 * args.rows * 64 * 64 * tiles * (tiles + 1) / 2
            out["cases"].append({
                "n_cols": d, "n_components": k, "layout": layout, "fit_ms": round(fit_ms, 3), "transform_ms": round(tr_ms, 3),
                "inverse_transform_ms": round(inv_ms, 3), "cov_kernel_ms": round(cov_ms, 3), "jacobi_ms": round(jac_ms, 3),
                "jacobi_sweeps": sweeps.value, "cov_tflops": round(flop / cov_ms / 1e9, 2) if cov_ms > 0 else None,
                "cov_share_of_fp32_mfma_peak": round(flop / cov_ms / 1e9 / FP32_MFMA_PEAK_TFLOPS, 4) if cov_ms > 0 else None
            })
            del X, t, y
        del base
    print(json.dumps(out))


if __name__ == "__main__":
    main()

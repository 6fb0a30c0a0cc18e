"""Exact Hamming kNN over packed bit codes against what there was before it: brute force over the 0/1-expanded rows.

    python scripts/bench_binary_knn.py [--rows 1000000] [--nbytes 128] [--queries 10000] [--k 10] [--out FILE.json]

Three lines. (1) binary_brute_force.knn on uniform random codes. (2) brute_force with sqeuclidean over the same rows expanded to
0/1 fp32 (32 times the bytes; squared L2 of 0/1 vectors is the Hamming distance, exact in fp32), whose ids and distances must equal
(1)'s. Both are the median wall time of `--steps` calls between two synchronisations after `--warmup` calls, the two alternating.
(3) the tile kernel alone, by the library's event timing in a run of its own: its 2 m n bits integer operations against the int8
matrix peak, and the codes it reads (every query block reads every code once) against the HBM peak."""
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
from cuvs_amd.neighbors import binary_brute_force, brute_force  # noqa: E402

PEAK_INT8_TOPS = 5033.2  # 256 CUs x 4 SIMDs x 2048 op/clk x 2.4 GHz (v_mfma_i32_32x32x32_i8: 65536 operations in 32 clocks)
HBM_PEAK_GBS = 8000.0    # MI355X HBM3E
QUERY_BLOCK = 128        # queries of a workgroup (kBQ of binary_knn.hip)


def expand(codes):
    """uint8 [n, nbytes] -> fp32 [n, 8 nbytes] of 0 / 1, in slabs"""
    out = torch.empty((codes.shape[0], codes.shape[1] * 8), dtype=torch.float32, device=codes.device)
    shifts = torch.arange(8, device=codes.device, dtype=torch.uint8)
    for r0 in range(0, codes.shape[0], 65536):
        c = codes[r0:r0 + 65536]
        out[r0:r0 + 65536] = ((c[:, :, None] >> shifts) & 1).reshape(c.shape[0], -1).float()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--nbytes", type=int, default=128)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = Resources()
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randint(0, 256, (a.rows, a.nbytes), dtype=torch.uint8, device="cuda", generator=gen)
    q = torch.randint(0, 256, (a.queries, a.nbytes), dtype=torch.uint8, device="cuda", generator=gen)
    xf, qf = expand(x), expand(q)
    index = brute_force.build(xf, metric="sqeuclidean", resources=res)
    runs = {"binary_knn": lambda: binary_brute_force.knn(x, q, a.k, resources=res),
            "brute_force_fp32_expanded": lambda: brute_force.search(index, qf, a.k, resources=res)}
    for _ in range(a.warmup):
        for run in runs.values():
            run()
    res.sync()
    times = {name: [] for name in runs}
    last = {}
    for _ in range(a.steps):
        for name, run in runs.items():
            t0 = time.perf_counter()
            last[name] = run()
            res.sync()
            times[name].append(time.perf_counter() - t0)
    same =all(torch.equal(u, v) for u, v in zip(last["binary_knn"], last["brute_force_fp32_expanded"]))
    ms = C.c_double(0)
    lib().cuvsAmdProfileCollect(b"bk_tile_kernel_fused", None)
    lib().cuvsAmdProfileEnable(1)
    runs["binary_knn"]()
    stats = binary_brute_force.last_stats(res)
    res.sync()
    lib().cuvsAmdProfileEnable(0)
    launches = lib().cuvsAmdProfileCollect(b"bk_tile_kernel_fused", C.byref(ms))
    ops = 2.0 * a.queries * a.rows * a.nbytes * 8
    read = float((a.queries + QUERY_BLOCK - 1) // QUERY_BLOCK) * a.rows * a.nbytes
    out = {"rows": a.rows, "nbytes": a.nbytes, "queries": a.queries, "k": a.k, "device": torch.cuda.get_device_name(0), "steps": a.steps,
           "warmup": a.warmup, "results_equal": same, "last_stats": stats, "tile_kernel_s": ms.value / 1e3, "tile_kernel_launches": launches,
           "tile_kernel_tops": ops / (ms.value / 1e3) / 1e12, "tile_kernel_share_of_int8_peak": ops / (ms.value / 1e3) / 1e12 / PEAK_INT8_TOPS,
           "tile_kernel_code_GBps": read / (ms.value / 1e3) / 1e9, "tile_kernel_share_of_hbm_peak": read / (ms.value / 1e3) / 1e9 / HBM_PEAK_GBS,
           "code_bytes": a.rows * a.nbytes, "expanded_bytes": a.rows * a.nbytes * 32}
    for name, t in times.items():
        out[name] = {"median_s": statistics.median(t), "min_s": min(t), "max_s": max(t), "queries_per_s": a.queries / statistics.median(t)}
        print("%-28s median %8.2f ms  (min %.2f, max %.2f)" % (name, 1e3 * out[name]["median_s"], 1e3 * min(t), 1e3 * max(t)), flush=True)
    out["speedup"] = out["brute_force_fp32_expanded"]["median_s"] / out["binary_knn"]["median_s"]
    print("results equal: %s   speedup %.1fx   tile kernel %.2f ms = %.0f TOP/s (%.1f %% of the int8 peak), codes at %.0f GB/s (%.1f %% of HBM)" %
          (same, out["speedup"], ms.value, out["tile_kernel_tops"], 100 * out["tile_kernel_share_of_int8_peak"], out["tile_kernel_code_GBps"],
           100 * out["tile_kernel_share_of_hbm_peak"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

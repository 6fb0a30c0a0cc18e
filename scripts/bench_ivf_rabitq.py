"""IVF-RaBitQ at 1M x 128 and 1M x 768 fp32 (n_lists 1024, n_probes 20, k 10, 10k queries) at 1, 3 and 5 bits per dimension in
the QUANT4 and QUANT8 modes: ms per batch, recall@10 against the library's brute force, bytes per row, screen survivors per
probed tail row, the screen kernel's time (HIP events around it) and its HBM bytes per second, and for context IVF-PQ on the same
rows at the nearest bytes per row. Prints one JSON line per dimension.

  python scripts/bench_ivf_rabitq.py [--dims 128 768] [--rows N] [--reps R] [--skip-pq]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs="+", default=[128, 768])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--n-lists", type=int, default=1024)
    ap.add_argument("--n-probes", type=int, default=20)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bits", type=int, nargs="+", default=[1, 3, 5])
    ap.add_argument("--skip-pq", action="store_true")
    a = ap.parse_args()
    from cuvs_amd._lib import lib
    from cuvs_amd.common import Resources
    from cuvs_amd.neighbors import brute_force, ivf_pq, ivf_rabitq

    res = Resources()

    def median_ms(fn, reps):
        fn()
        res.sync()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            res.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        return sorted(ts)[len(ts) // 2]

    def recall(found, truth):
        f, t = found.cpu().tolist(), truth.cpu().tolist()
        return round(sum(len(set(x) & set(y)) for x, y in zip(f, t)) / (len(t) * a.k), 4)

    for dim in a.dims:
        g = torch.Generator(device="cuda")
        g.manual_seed(dim)
        # clustered rows: blob centres + noise (uniform rows make every IVF index look the same)
        cent = torch.rand((a.n_lists, dim), generator=g, device="cuda")
        x = cent[torch.randint(0, a.n_lists, (a.rows,), generator=g, device="cuda")] + 0.15 * torch.randn(
            (a.rows, dim), generator=g, device="cuda")
        q = cent[torch.randint(0, a.n_lists, (a.queries,), generator=g, device="cuda")] + 0.15 * torch.randn(
            (a.queries, dim), generator=g, device="cuda")
        out = {"shape": f"{a.rows}x{dim} f32, n_lists {a.n_lists}, n_probes {a.n_probes}, {a.queries} queries, k {a.k}", "cases": []}
        _, truth = brute_force.search(brute_force.build(x, resources=res), q, a.k, resources=res)
        res.sync()
        D = (dim + 63) // 64 * 64
        for bits in a.bits:
            t0 = time.perf_counter()
            index = ivf_rabitq.build(ivf_rabitq.IndexParams(n_lists=a.n_lists, bits_per_dim=bits), x, resources=res)
            res.sync()
            build_s = round(time.perf_counter() - t0, 2)
            row_bytes = D * bits // 8 + 20  # codes + three short and two extended factors
            for mode in ("quant4", "quant8"):
                sp = ivf_rabitq.SearchParams(n_probes=a.n_probes, mode=mode)
                ms = median_ms(lambda: ivf_rabitq.search(sp, index, q, a.k, resources=res), a.reps)
                lib().cuvsAmdProfileEnable(1)
                _, nb = ivf_rabitq.search(sp, index, q, a.k, resources=res)
                res.sync()
                lib().cuvsAmdProfileEnable(0)
                scr, rsc = C.c_double(0), C.c_double(0)
                lib().cuvsAmdProfileCollect(b"rbq_screen_kernel", C.byref(scr))
                lib().cuvsAmdProfileCollect(b"rbq_rescore_kernel", C.byref(rsc))
                st = ivf_rabitq.last_search_stats()
                out["cases"].append({
                    "bits": bits, "mode": mode, "build_s": build_s, "ms_per_batch": round(ms, 3), "recall_at_10": recall(nb, truth),
                    "bytes_per_row": row_bytes, "survivors_per_tail_row": round(st["survivors"] / max(st["screened"], 1), 5),
                    "head_rows_per_query": round(st["head_rows"] / a.queries, 1), "screen_kernel_ms": round(scr.value, 3),
                    "rescore_kernels_ms": round(rsc.value, 3),
                    "screen_hbm_gb_per_s": round(st["screen_bytes"] / max(scr.value, 1e-9) / 1e6, 1)})
            if not a.skip_pq:
                pq_dim = max(8, min(dim, (row_bytes + 4) // 8 * 8))
                pq = ivf_pq.build(ivf_pq.IndexParams(n_lists=a.n_lists, pq_dim=pq_dim, pq_bits=8), x, resources=res)
                spq = ivf_pq.SearchParams(n_probes=a.n_probes)
                ms = median_ms(lambda: ivf_pq.search(spq, pq, q, a.k, resources=res), a.reps)
                _, nb = ivf_pq.search(spq, pq, q, a.k, resources=res)
                res.sync()
                out["cases"].append({"ivf_pq_for_bits": bits, "pq_dim": pq_dim, "bytes_per_row": pq_dim, "ms_per_batch": round(ms, 3),
                                     "recall_at_10": recall(nb, truth)})
                del pq
            del index
        print(json.dumps(out), flush=True)
        del x, q


if __name__ == "__main__":
    main()

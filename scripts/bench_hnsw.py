"""CAGRA -> HNSW hand-over, measured: the conversion by phase, the level-0 packing next to its two baselines, host
search throughput by thread count and recall next to cagra.search on the same graph.

  python scripts/bench_hnsw.py [--n 1000000 --dim 128 --degree 64 --queries 10000 --shm /dev/shm]

Packing baselines: (a) cuvsCagraSerializeToHnswlib to a memory-backed path - the host loop that interleaves the records and
writes them, what there was before cuvsHnsw*; (b) from_cagra(NONE) with CUVS_AMD_HNSW_PACK_HOST=1 - the same host loop into
the index's memory. from_cagra(NONE) is packing and nothing else; GPU minus NONE is the hierarchy. One JSON line per figure."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--degree", type=int, default=64)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--shm", default="/dev/shm")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()

    import torch

    import cuvs_amd
    from cuvs_amd._lib import check, lib
    from cuvs_amd.neighbors import brute_force, cagra, hnsw

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    rng = np.random.default_rng(0)
    x = rng.standard_normal((a.n, a.dim)).astype(np.float32)
    q = rng.standard_normal((a.queries, a.dim)).astype(np.float32)
    xd, qd = torch.from_numpy(x).cuda(), torch.from_numpy(q).cuda()
    res = cuvs_amd.common.Resources()

    t0 = time.perf_counter()
    ci = cagra.build(cagra.IndexParams(graph_degree=a.degree, intermediate_graph_degree=2 * a.degree), xd, resources=res)
    res.sync()
    emit(what="cagra.build", n=a.n, dim=a.dim, degree=a.degree, seconds=round(time.perf_counter() - t0, 3))

    def timed(f, reps=a.reps):
        best = None
        for _ in range(reps):
            t = time.perf_counter()
            out = f()
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
        return best, out

    # ---- packing: the export's host loop, the same loop into the index, the pack kernel
    path = os.path.join(a.shm, f"bench_hnsw_{os.getpid()}.bin")
    try:
        s, _ = timed(lambda: (check(lib().cuvsCagraSerializeToHnswlib(res.get_c_obj(), os.fsencode(path), ci._p)), res.sync()))
        emit(what="cuvsCagraSerializeToHnswlib (host loop + write to a memory-backed file)", seconds=round(s, 3),
             bytes=os.path.getsize(path))
    finally:
        if os.path.exists(path):
            os.remove(path)
    os.environ["CUVS_AMD_DEBUG_SWITCHES"] = "1"
    os.environ["CUVS_AMD_HNSW_PACK_HOST"] = "1"
    res_host = cuvs_amd.common.Resources()
    del os.environ["CUVS_AMD_HNSW_PACK_HOST"], os.environ["CUVS_AMD_DEBUG_SWITCHES"]
    s_host, _ = timed(lambda: hnsw.from_cagra(hnsw.IndexParams(hierarchy="none"), ci, resources=res_host))
    emit(what="from_cagra NONE, host loop (CUVS_AMD_HNSW_PACK_HOST=1)", seconds=round(s_host, 3))
    s_none, _ = timed(lambda: hnsw.from_cagra(hnsw.IndexParams(hierarchy="none"), ci, resources=res))
    emit(what="from_cagra NONE, pack kernel (packing phase)", seconds=round(s_none, 3))
    s_gpu, hi = timed(lambda: hnsw.from_cagra(hnsw.IndexParams(hierarchy="gpu"), ci, resources=res))
    emit(what="from_cagra GPU (packing + hierarchy)", seconds=round(s_gpu, 3), hierarchy_phase_seconds=round(s_gpu - s_none, 3))
    try:
        s, _ = timed(lambda: hnsw.save(path, hi), reps=1)
        emit(what="hnsw.save to a memory-backed file", seconds=round(s, 3), bytes=os.path.getsize(path))
    finally:
        if os.path.exists(path):
            os.remove(path)

    # ---- search: throughput by threads, recall next to cagra.search
    bf = brute_force.build(xd, resources=res)
    _, truth = brute_force.search(bf, qd, 10, resources=res)
    res.sync()
    truth = truth.cpu().numpy()

    def recall(got):
        return float(np.mean([len(set(g.tolist()) & set(t.tolist())) / 10.0 for g, t in zip(got, truth)]))

    for nt in (1, 4, 16):
        qs = q if nt > 1 else q[: max(1, a.queries // 4)]
        s, _ = timed(lambda: hnsw.search(hnsw.SearchParams(ef=64, num_threads=nt), hi, qs, 10), reps=2)
        emit(what="hnsw.search ef 64 k 10", threads=nt, queries=len(qs), qps=round(len(qs) / s, 1))
    for ef in (64, 200):
        _, hn = hnsw.search(hnsw.SearchParams(ef=ef, num_threads=16), hi, q, 10)
        _, cn = cagra.search(cagra.SearchParams(itopk_size=ef), ci, qd, 10, resources=res)
        res.sync()
        emit(what="recall@10", ef=ef, hnsw=round(recall(hn.astype(np.int64)), 4),
             cagra_itopk=round(recall(cn.cpu().numpy().view(np.uint32).astype(np.int64)), 4))


if __name__ == "__main__":
    main()

"""Binary quantizer and BitwiseHamming CAGRA next to fp32 L2 CAGRA. Prints one JSON line (profiles/binary_hamming_bench.json).

  * transform throughput of cuvsBinaryQuantizerTransformWithParams at 10M x 1024 fp32 rows (MEAN thresholds): GB/s of input
    and the HBM traffic (input + codes) as a fraction of the 8 TB/s peak;
  * a clustered 1M x 1024 fp32 corpus of intrinsic dimension 32, quantized (MEAN) to 1M x 128-byte codes: the CAGRA Hamming build (AUTO: NN-descent
    above 200000 rows) and the fp32 L2 CAGRA build over the same rows (the Python layer's default, IVF-PQ + refine), build
    time, then for each the search QPS and recall@10 at batch 10k, k 10, itopk 64, each against its own exact kNN
    (Hamming: tie-aware, a returned row counts when its distance is within the 10th exact distance).

  python scripts/binary_hamming_bench.py [--rows N] [--reps R] [--skip-transform] [--skip-l2]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--transform-rows", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-transform", action="store_true")
    ap.add_argument("--skip-l2", action="store_true")
    a = ap.parse_args()
    from cuvs_amd.common import Resources
    from cuvs_amd.neighbors import brute_force, cagra
    from cuvs_amd.preprocessing.quantize import binary

    res = Resources()
    out = {}

    def timed(fn, reps):
        fn()
        res.sync()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            res.sync()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ts.sort()
        return ts[len(ts) // 2]

    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    if not a.skip_transform:
        x = torch.empty((a.transform_rows, a.dim), device="cuda")
        for r0 in range(0, a.transform_rows, 1 << 20):
            x[r0:r0 + (1 << 20)].normal_(generator=g)
        q = binary.train(binary.QuantizerParams(threshold="mean"), x, resources=res)
        codes = torch.empty((a.transform_rows, a.dim // 8), dtype=torch.uint8, device="cuda")
        t = timed(lambda: binary.transform(x, output=codes, quantizer=q, resources=res), a.reps)
        in_b, out_b = x.numel() * 4, codes.numel()
        out["transform_shape"] = f"{a.transform_rows}x{a.dim} f32 -> {a.transform_rows}x{a.dim // 8} u8"
        out["transform_ms"] = round(t * 1e3, 3)
        out["transform_input_GBps"] = round(in_b / t / 1e9, 1)
        out["transform_hbm_fraction"] = round((in_b + out_b) / t / 1e9 / HBM_PEAK_GBS, 3)
        del x, codes
        torch.cuda.empty_cache()

    # clustered corpus of low intrinsic dimension: 256 cluster centres in a 32-d latent space, rows = latent points mapped to
    # 1024-d by a random linear map + isotropic noise (isotropic 1024-d blobs make every row about equally far from every
    # other of its blob - no index finds neighbours there); queries drawn the same way
    lat = 32
    w = torch.randn((lat, a.dim), generator=g, device="cuda") / lat ** 0.5
    cent = 3.0 * torch.randn((256, lat), generator=g, device="cuda")
    lab = torch.randint(0, 256, (a.rows + a.queries,), generator=g, device="cuda")
    z = cent[lab] + torch.randn((a.rows + a.queries, lat), generator=g, device="cuda")
    xf = z @ w + 0.1 * torch.randn((a.rows + a.queries, a.dim), generator=g, device="cuda")
    del lab, z
    xq, qf = xf[a.queries:].contiguous(), xf[:a.queries].contiguous()
    del xf
    qz = binary.train(binary.QuantizerParams(threshold="mean"), xq, resources=res)
    xb = binary.transform(xq, quantizer=qz, resources=res)
    qb = binary.transform(qf, quantizer=qz, resources=res)
    res.sync()
    out["corpus"] = f"{a.rows}x{a.dim} f32 clustered -> {a.rows}x{a.dim // 8} u8; {a.queries} queries, k {a.k}, itopk 64"
    sp = cagra.SearchParams(itopk_size=64)

    # exact Hamming kNN: 0/1 expansion, integer dot products (exact in fp32)
    shifts = torch.arange(8, device="cuda", dtype=torch.int32)

    def bits(v):
        return ((v.to(torch.int32)[:, :, None] >> shifts) & 1).reshape(v.shape[0], -1).float()

    xbits = bits(xb)
    xcnt = xbits.sum(1)
    kth = []
    for q0 in range(0, a.queries, 1000):
        qq = bits(qb[q0:q0 + 1000])
        d = qq.sum(1)[:, None] + xcnt[None, :] - 2.0 * (qq @ xbits.T)
        kth.append(torch.topk(d, a.k, dim=1, largest=False).values[:, -1:])
    kth = torch.cat(kth)
    del xbits, xcnt

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hidx = cagra.build(cagra.IndexParams(metric="bitwise_hamming", build_algo="auto"), xb, resources=res)
    res.sync()
    out["hamming_build_s"] = round(time.perf_counter() - t0, 2)
    t = timed(lambda: cagra.search(sp, hidx, qb, a.k, resources=res), a.reps)
    out["hamming_search_ms"] = round(t * 1e3, 3)
    out["hamming_qps"] = round(a.queries / t)
    d, i = cagra.search(sp, hidx, qb, a.k, resources=res)
    res.sync()
    out["hamming_recall_at_10_tie_aware"] = round(float((d <= kth).float().mean().item()), 4)
    del hidx

    if not a.skip_l2:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lidx = cagra.build(cagra.IndexParams(metric="sqeuclidean"), xq, resources=res)
        res.sync()
        out["l2_build_s"] = round(time.perf_counter() - t0, 2)
        t = timed(lambda: cagra.search(sp, lidx, qf, a.k, resources=res), a.reps)
        out["l2_search_ms"] = round(t * 1e3, 3)
        out["l2_qps"] = round(a.queries / t)
        _, li = cagra.search(sp, lidx, qf, a.k, resources=res)
        bf = brute_force.build(xq, resources=res)
        _, ti = brute_force.search(bf, qf, a.k, resources=res)
        res.sync()
        li, ti = (li.to(torch.int64) & 0xFFFFFFFF).cpu(), ti.cpu()
        hits = sum(len(set(li[r].tolist()) & set(ti[r].tolist())) for r in range(a.queries))
        out["l2_recall_at_10"] = round(hits / (a.queries * a.k), 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

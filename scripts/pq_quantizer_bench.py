"""Product and scalar quantizer timings on device-resident rows. Writes one JSON (profiles/pq_quantizer_bench.json).

  * product quantizer: Build (wall clock of the synchronous call), Transform through the default encoder and through the plain
    one (CUVS_AMD_PQ_ENCODE=plain on a second handle of the same process), InverseTransform; the kernels are timed with HIP
    events on the handle's stream (cuvsAmdProfileEnable / cuvsAmdProfileCollect), median of --reps after one warm-up;
  * scalar quantizer: Transform and InverseTransform at 10M x 1024 fp32 and fp16.
  Per line: milliseconds, GB/s of unique bytes (rows + codes), distance evaluations per second and those at 3 pq_len flop each
  as a fraction of the 157.3 TFLOP/s fp32 peak.

  python scripts/pq_quantizer_bench.py [--reps R] [--quick] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0    # MI355X HBM3E
FP32_PEAK_TFLOPS = 157.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="a tenth of the rows")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from cuvs_amd._lib import lib
    from cuvs_amd.common import Resources
    from cuvs_amd.preprocessing.quantize import pq, scalar

    L = lib()
    res = Resources()
    os.environ["CUVS_AMD_DEBUG_SWITCHES"] = "1"
    os.environ["CUVS_AMD_PQ_ENCODE"] = "plain"
    res_plain = Resources()  # the switches are read when a handle is created
    del os.environ["CUVS_AMD_PQ_ENCODE"], os.environ["CUVS_AMD_DEBUG_SWITCHES"]
    L.cuvsAmdProfileEnable(1)

    def kernel_ms(name, fn, reps):
        ms = C.c_double()
        fn()
        L.cuvsAmdProfileCollect(name.encode(), C.byref(ms))
        ts = []
        for _ in range(reps):
            fn()
            assert L.cuvsAmdProfileCollect(name.encode(), C.byref(ms)) >= 1, name
            ts.append(ms.value)
        return sorted(ts)[len(ts) // 2], ts

    scale = 10 if a.quick else 1
    g = torch.Generator(device="cuda").manual_seed(0)
    lines = []
    # (rows, dim, pq_dim, pq_bits, use_vq, time the build)
    shapes = [(1_000_000, 128, 32, 8, False, True), (1_000_000, 128, 64, 8, False, False), (1_000_000, 768, 192, 8, False, False),
              (1_000_000, 1024, 128, 8, False, True), (1_000_000, 1024, 128, 5, False, False), (1_000_000, 1024, 128, 8, True, True),
              (200_000, 1024, 128, 12, False, False)]
    for n, dim, pq_dim, bits, vq, do_build in shapes:
        n //= scale
        x = torch.randn((n, dim), generator=g, device="cuda")
        pq_len, book_n = dim // pq_dim, 1 << bits
        line = {"op": "pq", "shape": f"{n}x{dim} f32", "pq_dim": pq_dim, "pq_bits": bits, "pq_len": pq_len, "use_vq": vq}
        params = pq.QuantizerParams(pq_bits=bits, pq_dim=pq_dim, use_vq=vq, vq_n_centers=1024 if vq else 0)
        if do_build:
            t0 = time.perf_counter()
            q = pq.build(params, x, resources=res)
            res.sync()
            line["build_s"] = round(time.perf_counter() - t0, 3)
        else:  # the encoder's time does not depend on how the books were trained
            q = pq.from_codebooks(params, torch.randn((pq_dim * book_n, pq_len), generator=g, device="cuda"), resources=res)
        codes = torch.empty((n, q.encoded_dim), dtype=torch.uint8, device="cuda")
        labels = torch.empty((n,), dtype=torch.uint32, device="cuda") if vq else None
        evals = n * pq_dim * book_n
        unique_gb = (n * dim * 4 + codes.numel()) / 1e9
        # which encoder the library's rule gives this shape: asked of the launch counters, not restated here
        cnt0, cnt1 = (C.c_ulonglong * 3)(), (C.c_ulonglong * 3)()
        L.cuvsAmdPqEncodeCounters(cnt0)
        pq.transform(q, x, codes_output=codes, vq_labels=labels, resources=res)
        L.cuvsAmdPqEncodeCounters(cnt1)
        use_default = cnt1[0] > cnt0[0]
        line["rows_per_lane_gt_1"] = bool(cnt1[2] > cnt0[2])
        ms_d, all_d = kernel_ms("pq_encode_kernel" if use_default else "pq_encode_plain_kernel",
                                lambda: pq.transform(q, x, codes_output=codes, vq_labels=labels, resources=res), a.reps)
        ref = codes.clone()
        ms_p, all_p = kernel_ms("pq_encode_plain_kernel", lambda: pq.transform(q, x, codes_output=codes, vq_labels=labels, resources=res_plain),
                                a.reps)
        assert torch.equal(ref, codes), "default and plain encoders differ"
        for tag, ms, runs in (("default", ms_d, all_d), ("plain", ms_p, all_p)):
            line[f"transform_{tag}_ms"] = round(ms, 3)
            line[f"transform_{tag}_runs_ms"] = [round(v, 3) for v in runs]
            line[f"transform_{tag}_GBps"] = round(unique_gb / (ms / 1e3), 1)
            line[f"transform_{tag}_evals_per_s"] = float(f"{evals / (ms / 1e3):.4g}")
            line[f"transform_{tag}_fp32_peak_fraction"] = round(evals * 3 * pq_len / (ms / 1e3) / (FP32_PEAK_TFLOPS * 1e12), 4)
        line["plain_over_default"] = round(ms_p / ms_d, 2)
        out = torch.empty((n, dim), device="cuda")
        ms_i, _ = kernel_ms("pq_decode_kernel", lambda: pq.inverse_transform(q, codes, out, vq_labels=labels, resources=res), a.reps)
        line["inverse_ms"] = round(ms_i, 3)
        line["inverse_GBps"] = round(unique_gb / (ms_i / 1e3), 1)
        line["inverse_hbm_fraction"] = round(unique_gb / (ms_i / 1e3) / HBM_PEAK_GBS, 3)
        lines.append(line)
        print(json.dumps(line), flush=True)
        del x, out, codes, ref, q
        torch.cuda.empty_cache()

    n = 10_000_000 // scale
    for dtype in (torch.float32, torch.float16):
        x = torch.empty((n, 1024), device="cuda", dtype=dtype)
        for r0 in range(0, n, 1 << 20):
            x[r0:r0 + (1 << 20)] = torch.randn((min(1 << 20, n - r0), 1024), generator=g, device="cuda").to(dtype)
        q = scalar.train(scalar.QuantizerParams(), x, resources=res)
        codes = torch.empty((n, 1024), dtype=torch.int8, device="cuda")
        gb = (x.numel() * x.element_size() + codes.numel()) / 1e9
        ms_t, _ = kernel_ms("sq_transform_kernel", lambda: scalar.transform(q, x, output=codes, resources=res), a.reps)
        ms_i, _ = kernel_ms("sq_inverse_kernel", lambda: scalar.inverse_transform(q, codes, output=x, resources=res), a.reps)
        line = {"op": "scalar", "shape": f"{n}x1024 {str(dtype).replace('torch.', '')}", "transform_ms": round(ms_t, 3),
                "transform_GBps": round(gb / (ms_t / 1e3), 1), "transform_hbm_fraction": round(gb / (ms_t / 1e3) / HBM_PEAK_GBS, 3),
                "inverse_ms": round(ms_i, 3), "inverse_GBps": round(gb / (ms_i / 1e3), 1),
                "inverse_hbm_fraction": round(gb / (ms_i / 1e3) / HBM_PEAK_GBS, 3)}
        lines.append(line)
        print(json.dumps(line), flush=True)
        del x, codes
        torch.cuda.empty_cache()
    path = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pq_quantizer_bench.json")
    with open(path, "w") as f:
        json.dump({"lines": lines}, f)
        f.write("\n")


if __name__ == "__main__":
    main()

"""CPU: the IVF-PQ search plan (host arithmetic only, no GPU) - which path a search takes, its modifiers and its sizes - pinned
against an independent Python transcription of the dispatch rules as they stood before the plan was factored out of
ivf_pq_search (commit bd07b0a). Line numbers below cite THAT commit:
  ivf_pq_search.hip:313-331 (scan_layout), :1747-1753 (scan_smem_bytes), :2075-2301 (the search's decisions and sizes);
  ivf_pq_scan3.hip:2561-2569 (pq3_supported), :2576-2590 (pq3_bound_useful), :2651-2660 (pq3_max_units),
  :3104-3108 (pqw_supported), :3110-3120 (pqw_heads); ivf_pq_wide.hip:479-482 (pqw_shape);
  common.hpp:349-356 (balanced_batch); ivf_common.hpp:178-186 (largest_lists_total).
The hook runs with the production tuning (no CUVS_AMD_* switch) and no communicator."""
import ctypes as C

import numpy as np
import pytest

LUT_ONE_PHASE, LUT_TWO_PHASE, SCAN2_TAIL, MATRIX_CORE_TAIL, WIDE, ALL_SCORES = range(6)
L2, COSINE, IP = 0, 2, 6  # cuvsDistanceType values (common.hpp:322-323)
F32, F16, FP8 = np.float32, np.float16, np.uint8

# production tuning (common.hpp: struct tuning defaults)
T = dict(pq_head_probes=-1, pq_scan2=1, pq_scan3=1, pq_head_rows=-1, pq_overlap=1, pq_filter4=1, pq_wide=1, pq_wide_heads=0,
         pq3_surv_cap=0, shard_coarse_replicated=False)
KEYS = ["path", "glut", "head1", "overlap", "big_k", "filter4", "qpb", "smem", "k_scan", "head", "wheads", "head_rows",
        "max_list_len", "w_ldx", "n_ranges", "n_labels", "max_batch", "bs_alloc", "surv_cap", "overflow_cap", "max_units",
        "unit_rows", "max_items", "shard_coarse"]


def plan_hook(shape, sizes, k, nq, *, n_probes, lut=F32, score=F32, batch=4096, num_cus=256, limit=8 << 30, ready=True):
    from cuvs_amd._lib import check, lib
    from cuvs_amd.neighbors import ivf_pq

    sp = ivf_pq.SearchParams(n_probes=n_probes, lut_dtype=lut, internal_distance_dtype=score, max_internal_batch_size=batch)
    s = np.ascontiguousarray(sizes, dtype=np.uint32)
    out = (C.c_int64 * 24)()
    fn = lib().cuvsAmdIvfPqSearchPlan
    fn.argtypes = [C.c_uint32] * 6 + [C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int,
                                      C.c_uint64, C.c_int, C.c_void_p]
    check(fn(shape["dim"], shape["rot_dim"], shape["pq_dim"], shape["pq_len"], shape["pq_bits"], shape.get("world", 1),
             shape.get("kind", 0), shape.get("metric", L2), len(s), s.ctypes.data, sp._p, k, nq, num_cus, limit, int(ready),
             out))
    return dict(zip(KEYS, list(out)))


# ---------------------------------------------------------------- transcription of the parent commit's rules
def r16(x):
    return (x + 15) & ~15


def round_up(a, b):
    return (a + b - 1) // b * b


def scan_layout_total(lut_bytes, qpb, rot_dim, k):  # ivf_pq_search.hip:313-331 (kScanWaves 16, kQueueRows 320)
    off = r16(lut_bytes)
    mg = qpb * 16 * k * 8
    if k > 64:
        mg = max(mg, 16 * 256 * 8)
    if mg > off:
        off = r16(mg)
    off += r16(qpb * rot_dim * 4)
    off += r16(rot_dim * 4)
    off += 16 * 4 + 16 * 4 + 2 * 16
    off += 16 * 320 * 4
    return off


def scan_smem_bytes(sh, esz, qpb, k):  # :1747-1753; esz = sizeof(lut_acc<LutT, AccT, QPB>::entry_t)
    fast4 = sh["pq_bits"] == 8 and sh["pq_dim"] == 64
    lut = 256 * (64 * esz + 8) if fast4 else sh["pq_dim"] * (1 << sh["pq_bits"]) * esz  # cm_lut::bytes()
    return scan_layout_total(lut, qpb, sh["rot_dim"], k)


def pq3_supported(sh, k):  # ivf_pq_scan3.hip:2561-2569
    return (4 <= sh["pq_bits"] <= 8 and sh["pq_len"] in (1, 2, 4, 8) and sh["pq_dim"] % 16 == 0 and 16 <= sh["pq_dim"] <= 128
            and sh["rot_dim"] == sh["pq_len"] * sh["pq_dim"] and sh["rot_dim"] <= 256 and k <= 256)


def pq3_bound_useful(sizes, k):  # :2576-2590 (no communicator: the index's own lists)
    rows, lists = int(np.sum(sizes, dtype=np.uint64)), int(np.count_nonzero(sizes))
    return lists != 0 and k * 25 * lists <= rows


def pq3_max_units(sizes, n_pairs, filter4):  # :2651-2660 -> (units, unit_rows)
    max_len = int(np.max(sizes))
    ur = max(8192 if filter4 else 4096, round_up((max_len + 15) // 16, 64))
    return 16 * (n_pairs // 32 + len(sizes) + 1), ur


def pqw_shape(rot_dim):  # ivf_pq_wide.hip:479-482
    return rot_dim in (64, 96, 128, 256, 384, 512, 768)


def pqw_supported(sh, k):  # ivf_pq_scan3.hip:3104-3108
    return (sh.get("kind", 0) == 0 and 4 <= sh["pq_bits"] <= 8 and sh["pq_dim"] % 16 == 0 and sh["pq_dim"] >= 16
            and sh["rot_dim"] == sh["pq_len"] * sh["pq_dim"] and pqw_shape(sh["rot_dim"]) and k <= 256 and sh.get("world", 1) <= 1)


def pqw_heads(sizes, k, n_probes):  # :3110-3120
    rows, lists = int(np.sum(sizes, dtype=np.uint64)), int(np.count_nonzero(sizes))
    if lists == 0 or rows == 0:
        return 0
    h = max(1, (40 * k * lists + rows - 1) // rows)
    return h if 2 * h <= n_probes else 0


def balanced_batch(n, fit):  # common.hpp:349-356
    fit = max(1, fit)
    if n <= fit:
        return max(n, 1)
    nb = (n + fit - 1) // fit
    return (n + nb - 1) // nb


def largest_lists_total(sizes, n_probes):  # ivf_common.hpp:178-186
    return int(np.sort(np.asarray(sizes, np.int64))[::-1][:n_probes].sum())


def ref_plan(sh, sizes, k, nq, *, n_probes, lut=F32, score=F32, batch=4096, num_cus=256, limit=8 << 30, ready=True):
    sizes = np.asarray(sizes, np.int64)
    n_lists, rot_dim, dim = len(sizes), sh["rot_dim"], sh["dim"]
    metric, kind, pq_len, world = sh.get("metric", L2), sh.get("kind", 0), sh["pq_len"], sh.get("world", 1)
    lut_dtype = {F32: 0, F16: 2, FP8: 8}[lut]
    idd = {F32: 0, F16: 2}[score]
    # ivf_pq_search.hip:2075-2084
    n_probes = min(n_probes, n_lists)
    lut_fp8 = lut_dtype in (8, 3)
    acc_half = lut_dtype != 0 and idd == 2
    lut_half = acc_half if lut_fp8 else lut_dtype != 0
    large_k = k > 256
    big_k = k > 64 and not large_k
    k_scan = 1 if large_k else k
    # :2086-2103 the widest interleave whose LUT fits 160 KiB (entry bytes: fp32 x qpb, fp16 x qpb)
    qpb, smem = 0, 0
    for q in ((2, 1) if not lut_half else (4, 2, 1)):
        smem = scan_smem_bytes(sh, (2 if lut_half else 4) * q, q, k_scan)
        if smem <= 160 * 1024:
            qpb = q
            break
    glut = qpb == 0
    if glut:
        qpb = 4 if lut_half else 2
        smem = scan_layout_total(0, qpb, rot_dim, k_scan)
    # :2109
    largest_total = largest_lists_total(sizes, n_probes) if large_k else 0
    # :2117-2129 the wide path
    mc = pq3_supported(sh, k) and pq3_bound_useful(sizes, k) and ((pq_len == 2 and kind == 0) or T["pq_filter4"] != 0)
    wheads = 0
    if (not large_k and n_probes > 8 and nq >= 256 and T["pq_scan3"] != 0 and T["pq_wide"] != 0 and T["pq_head_probes"] < 0
            and world <= 1 and pqw_supported(sh, k) and not mc):
        wheads = min(T["pq_wide_heads"], n_probes // 2) if T["pq_wide_heads"] > 0 else pqw_heads(sizes, k, n_probes)
        if wheads > 0 and not ready:
            wheads = 0
    usew = wheads > 0
    # :2133-2135
    max_list_len = int(sizes.max())
    w_ldx = round_up(max_list_len + 64, 64) if usew else 0
    # :2137-2150 the per-query budget
    max_batch = max(1, batch)
    per_q = n_lists * 4 + n_probes * k_scan * 8 + rot_dim * 4 + dim * 4
    if large_k:
        per_q += largest_total * 8
    if not large_k and (pq3_supported(sh, k) or usew) and T["pq_scan3"] != 0:
        per_q += n_probes * (rot_dim * 2 + k * 4 + 128 + 16 + 4 + 16 + 8)
    if usew:
        per_q += wheads * (w_ldx * 4 + 32) + k * (8 + 32 * 8)
    fit = max(1, limit // per_q)
    max_batch = balanced_batch(nq, min(max_batch, fit))
    bs_alloc = min(max_batch, nq)
    n_pairs_max = bs_alloc * n_probes
    # :2162-2172 the head phase and the labels
    head = 1 if (n_probes > 8 and nq >= 256 and not large_k) else 0
    if T["pq_head_probes"] >= 0:
        head = min(T["pq_head_probes"], n_probes)
    pq3_ok = (not large_k and pq3_supported(sh, k) and pq3_bound_useful(sizes, k) and T["pq_scan3"] != 0
              and T["pq_head_probes"] != 0 and ((pq_len == 2 and kind == 0) or T["pq_filter4"] != 0))
    if metric in (IP, COSINE) and not pq3_ok:
        head = 0
    if usew:
        head = wheads
    sharded = world > 1
    n_ranges = 2 * n_lists if head > 0 else n_lists
    n_labels = n_ranges + (1 if sharded else 0)
    max_items = n_pairs_max // qpb + bs_alloc * head + n_labels + 1  # :2178
    # :2191-2209 the matrix-core tail
    use3 = (not usew and head > 0 and not large_k and pq3_supported(sh, k) and pq3_bound_useful(sizes, k) and T["pq_scan3"] != 0
            and ((pq_len == 2 and kind == 0) or T["pq_filter4"] != 0))
    use3x = use3 or usew
    not_pqf = metric != IP or pq_len != 2 or kind != 0
    max_units, unit_rows = 0, 0
    if usew:
        max_units, unit_rows = pq3_max_units(sizes, n_pairs_max, False)
    elif use3:
        max_units, unit_rows = pq3_max_units(sizes, n_pairs_max, T["pq_filter4"] != 0 and not_pqf)
    surv_cap = min(max(n_pairs_max * 16, 1 << 22), 1 << 28) if use3x else 0
    if usew:
        surv_cap = min(max(surv_cap, bs_alloc * k * 32), 1 << 28)
    overflow_cap = (1 << 22) if use3x else 0
    use_f4 = use3 and T["pq_filter4"] != 0 and not_pqf
    # :2220 two-stream schedule, :2246-2251 partial head (default rule: 0)
    overlap = use3 and use_f4 and head == 1 and not glut and T["pq_overlap"] != 0
    head_rows = 0
    if overlap and T["pq_head_rows"] >= 0:
        head_rows = T["pq_head_rows"] // 64 * 64
        if head_rows != 0 and head_rows < 4 * k:
            head_rows = 0
    # :2293-2295 the pq_scan2 tail, :2301 single-pair head items
    bits8 = sh["pq_bits"] == 8 and sh["pq_dim"] == 64
    use2 = (head > 0 and bits8 and pq_len == 2 and kind == 0 and k <= 64 and ((lut_half and qpb == 4) or (not lut_half and qpb == 2))
            and T["pq_scan2"] != 0 and not use3x)
    lut_bytes = 4 if (lut_dtype == 0 or (lut_fp8 and not acc_half)) else 2
    head1 = (use3 and not glut) or (usew and not glut and rot_dim <= 256 and sh["pq_dim"] * 256 * lut_bytes <= 96 * 1024)
    # the path: the booleans the batch loop reads together (:2285-2511)
    if large_k:
        path = ALL_SCORES
    elif usew:
        path = WIDE
    elif use3:
        path = MATRIX_CORE_TAIL
    elif head == 0:
        path = LUT_ONE_PHASE
    elif use2:
        path = SCAN2_TAIL
    else:
        path = LUT_TWO_PHASE
    shard_coarse = False  # :2262-2263 (no communicator)
    vals = [path, glut, head1, overlap, big_k, use_f4, qpb, smem, k_scan, head, wheads, head_rows, max_list_len, w_ldx, n_ranges,
            n_labels, max_batch, bs_alloc, surv_cap, overflow_cap, max_units, unit_rows, max_items, shard_coarse]
    return dict(zip(KEYS, [int(v) for v in vals]))


# ---------------------------------------------------------------- the table
def sizes_of(n_lists, mean, seed=0, spread=0.5):
    rng = np.random.default_rng(seed)
    return np.maximum(0, rng.normal(mean, spread * mean, n_lists)).astype(np.uint32)


H128 = dict(dim=128, rot_dim=128, pq_dim=64, pq_len=2, pq_bits=8)  # the headline C3 index: 100M rows, 16384 lists
C3 = sizes_of(16384, 6100)
D768 = dict(dim=768, rot_dim=768, pq_dim=384, pq_len=2, pq_bits=8)  # the reference's default pq_dim at 768 dimensions
CAGRA768 = dict(dim=768, rot_dim=768, pq_dim=64, pq_len=12, pq_bits=8)  # knn_graph_ivf_pq at 2M x 768: 1414 lists, 28 probes
CAGRA128 = dict(dim=128, rot_dim=128, pq_dim=64, pq_len=2, pq_bits=8)  # knn_graph_ivf_pq at 1M x 128: 1000 lists, 20 probes
GIST = dict(dim=960, rot_dim=960, pq_dim=480, pq_len=2, pq_bits=8)

CASES = {
    # the headline (bench.py): every LUT / score type
    "c3_k10_f32": (H128, C3, 10, 10000, dict(n_probes=128)),
    "c3_k10_f16lut": (H128, C3, 10, 10000, dict(n_probes=128, lut=F16)),
    "c3_k10_f16lut_f16": (H128, C3, 10, 10000, dict(n_probes=128, lut=F16, score=F16)),
    "c3_k20_f16lut": (H128, C3, 20, 10000, dict(n_probes=128, lut=F16)),
    "c3_k20_f32": (H128, C3, 20, 10000, dict(n_probes=128)),
    "c3_k10_fp8": (H128, C3, 10, 10000, dict(n_probes=128, lut=FP8)),
    "c3_k10_fp8_f16": (H128, C3, 10, 10000, dict(n_probes=128, lut=FP8, score=F16)),
    "c3_k10_small_limit": (H128, C3, 10, 10000, dict(n_probes=128, lut=F16, limit=64 << 20)),
    "c3_k10_tiny_limit": (H128, C3, 10, 10000, dict(n_probes=128, limit=1 << 20)),
    # inner product at pq_len 2 (pq_filter_kernel), cosine, PER_CLUSTER
    "ip_pqlen2": (dict(H128, metric=IP), C3, 10, 10000, dict(n_probes=128, lut=F16)),
    "cosine": (dict(H128, metric=COSINE), C3, 10, 10000, dict(n_probes=128, lut=F16)),
    "ip_pqlen4": (dict(dim=128, rot_dim=128, pq_dim=32, pq_len=4, pq_bits=8, metric=IP), sizes_of(1024, 4000), 10, 5000,
                  dict(n_probes=64)),
    "per_cluster": (dict(H128, kind=1), sizes_of(2048, 3000), 10, 5000, dict(n_probes=64, lut=F16)),
    "per_cluster_ip": (dict(H128, kind=1, metric=IP), sizes_of(2048, 3000), 10, 5000, dict(n_probes=64)),
    # codes of 4 .. 7 bits
    **{f"bits{b}": (dict(H128, pq_bits=b), sizes_of(1024, 5000, seed=b), 10, 4000, dict(n_probes=32, lut=F16)) for b in (4, 5, 6, 7)},
    "bits5_pqdim32": (dict(dim=96, rot_dim=96, pq_dim=32, pq_len=3, pq_bits=5), sizes_of(512, 3000), 10, 2000, dict(n_probes=16)),
    # no head phase: fewer than 256 queries, n_probes <= 8
    "few_queries": (H128, C3, 10, 200, dict(n_probes=128, lut=F16)),
    "few_queries_f32": (H128, C3, 10, 255, dict(n_probes=128)),
    "eight_probes": (H128, C3, 10, 10000, dict(n_probes=8, lut=F16)),
    "eight_probes_ip": (dict(H128, metric=IP), C3, 10, 10000, dict(n_probes=8)),
    # LUT too large for LDS: the global-memory LUT
    "glut_f32": (dict(dim=256, rot_dim=256, pq_dim=128, pq_len=2, pq_bits=8), sizes_of(1024, 3000), 10, 3000, dict(n_probes=32)),
    "glut_f16": (dict(dim=512, rot_dim=512, pq_dim=256, pq_len=2, pq_bits=8), sizes_of(1024, 3000), 10, 3000,
                 dict(n_probes=32, lut=F16)),
    "glut_ip_small_batch": (dict(dim=512, rot_dim=512, pq_dim=256, pq_len=2, pq_bits=8, metric=IP), sizes_of(256, 800), 32, 100,
                            dict(n_probes=16)),
    # k = 100 of ~1k-row lists: the head bound is not useful
    "k100_short_lists": (H128, sizes_of(4096, 1000), 100, 5000, dict(n_probes=64, lut=F16)),
    "k100_short_lists_nowide": (H128, sizes_of(4096, 1000), 100, 5000, dict(n_probes=64, lut=F16, ready=False)),
    "k100_long_lists": (H128, C3, 100, 5000, dict(n_probes=64, lut=F16)),
    "k64_scan2_edge": (H128, C3, 64, 5000, dict(n_probes=64, lut=F16)),
    # the pq_scan2 tail: a bound that is not useful and no wide path
    "scan2_f16": (H128, sizes_of(4096, 1000), 64, 5000, dict(n_probes=64, lut=F16, ready=False)),
    "scan2_f32": (H128, sizes_of(4096, 1000), 48, 5000, dict(n_probes=64, ready=False)),
    "scan2_fp8_f16": (H128, sizes_of(4096, 1000), 64, 5000, dict(n_probes=64, lut=FP8, score=F16, ready=False)),
    # the wide path: 768-d rows, the CAGRA build's searches - and the same without room for the decoded rows
    "d768": (D768, sizes_of(1024, 1000), 10, 10000, dict(n_probes=32)),
    "d768_f16": (D768, sizes_of(1024, 1000), 10, 10000, dict(n_probes=32, lut=F16)),
    "d768_not_ready": (D768, sizes_of(1024, 1000), 10, 10000, dict(n_probes=32, ready=False)),
    "cagra768": (CAGRA768, sizes_of(1414, 1414), 256, 16384, dict(n_probes=28, lut=F16, batch=16384)),
    "cagra768_k130": (CAGRA768, sizes_of(1414, 1414), 130, 16384, dict(n_probes=28, lut=F16, batch=16384)),
    "cagra768_not_ready": (CAGRA768, sizes_of(1414, 1414), 256, 16384, dict(n_probes=28, lut=F16, batch=16384, ready=False)),
    "cagra128": (CAGRA128, sizes_of(1000, 1000), 130, 16384, dict(n_probes=20, lut=F16, score=F16, batch=16384)),
    "cagra128_not_ready": (CAGRA128, sizes_of(1000, 1000), 130, 16384,
                           dict(n_probes=20, lut=F16, score=F16, batch=16384, ready=False)),
    "wide_cosine_fp8": (dict(D768, metric=COSINE), sizes_of(1024, 1000), 10, 10000, dict(n_probes=32, lut=FP8)),
    # all-scores path beyond k = 256
    "k257": (H128, sizes_of(1024, 3000), 257, 2000, dict(n_probes=32, lut=F16)),
    "k320": (H128, sizes_of(1024, 3000), 320, 2000, dict(n_probes=32)),
    "k320_small_limit": (H128, sizes_of(1024, 3000), 320, 2000, dict(n_probes=32, limit=256 << 20)),
    # gist: rot_dim 960 stays on the LUT scan
    "gist": (GIST, sizes_of(1000, 1000), 10, 1000, dict(n_probes=32)),
    "gist_f16": (GIST, sizes_of(1000, 1000), 10, 1000, dict(n_probes=32, lut=F16)),
    # a list shard (two ranks, no communicator): foreign lists are empty, pairs on them go to one extra label
    "shard_world2": (dict(H128, world=2), np.where(np.arange(16384) % 2 == 0, C3, 0), 10, 10000, dict(n_probes=128, lut=F16)),
    "shard_world2_ip": (dict(H128, world=2, metric=IP), np.where(np.arange(16384) % 2 == 0, C3, 0), 10, 10000,
                        dict(n_probes=128)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_equals_the_transcribed_rules(name):
    sh, sizes, k, nq, kw = CASES[name]
    got, want = plan_hook(sh, sizes, k, nq, **kw), ref_plan(sh, sizes, k, nq, **kw)
    assert got == want, {key: (got[key], want[key]) for key in KEYS if got[key] != want[key]}


def test_table_reaches_every_path_and_modifier():
    plans = [ref_plan(sh, sizes, k, nq, **kw) for sh, sizes, k, nq, kw in CASES.values()]
    assert {p["path"] for p in plans} == set(range(6))
    for key in ("glut", "head1", "overlap", "big_k", "filter4"):
        assert {p[key] for p in plans} == {0, 1}, key


def test_headline_pins():
    p = plan_hook(H128, C3, 10, 10000, n_probes=128, lut=F16)
    assert p["path"] == MATRIX_CORE_TAIL and p["overlap"] and p["filter4"] and p["head1"] and p["head"] == 1
    assert p["max_batch"] == 3334 and p["bs_alloc"] == 3334 and p["qpb"] == 4
    small = plan_hook(H128, C3, 10, 10000, n_probes=128, lut=F16, limit=64 << 20)
    per_q = 16384 * 4 + 128 * 10 * 8 + 128 * 4 + 128 * 4 + 128 * (128 * 2 + 10 * 4 + 128 + 16 + 4 + 16 + 8)
    assert small["max_batch"] == balanced_batch(10000, (64 << 20) // per_q) == 477

"""CPU: the tiered index's C ABI (struct layouts, enum values, defaults, exported symbols) and self-checks of the numpy
restatement tests/tiered_index_ref.py (the merge rule against a plain sort, the growth policy, the bitset slice)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import tiered_index_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cuvs_amd", "libcuvs_c.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_struct_layouts_match_the_reference_headers(tmp_path):
    # tests/golden/tiered_index_abi_layout.txt: the same probe compiled against the reference's c/include
    # (gen_tiered_index_abi_layout.sh)
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(GOLDEN, "tiered_index_abi_probe.c"), "-o",
                           str(exe)])
    assert subprocess.check_output([str(exe)]).decode() == open(os.path.join(GOLDEN, "tiered_index_abi_layout.txt")).read()


def test_ctypes_mirror_has_the_layout_of_the_header():
    from cuvs_amd.neighbors import tiered_index as T

    want = dict(line.rsplit(" ", 1) for line in open(os.path.join(GOLDEN, "tiered_index_abi_layout.txt")).read().splitlines())
    assert C.sizeof(T._CIndex) == int(want["sizeof cuvsTieredIndex"])
    assert C.sizeof(T._CIndexParams) == int(want["sizeof struct cuvsTieredIndexParams"])
    for f in ("addr", "dtype", "algo"):
        assert getattr(T._CIndex, f).offset == int(want[f"offsetof cuvsTieredIndex.{f}"])
    for f, _ in T._CIndexParams._fields_:
        assert getattr(T._CIndexParams, f).offset == int(want[f"offsetof struct cuvsTieredIndexParams.{f}"])
    assert T.ALGO_TYPES == {"cagra": int(want["value CUVS_TIERED_INDEX_ALGO_CAGRA"]),
                            "ivf_flat": int(want["value CUVS_TIERED_INDEX_ALGO_IVF_FLAT"]),
                            "ivf_pq": int(want["value CUVS_TIERED_INDEX_ALGO_IVF_PQ"])}


def test_symbols_exported_and_defaults_match_the_reference():
    from cuvs_amd.neighbors import tiered_index as T

    lib = C.CDLL(LIB)
    for s in ("cuvsTieredIndexCreate", "cuvsTieredIndexDestroy", "cuvsTieredIndexParamsCreate", "cuvsTieredIndexParamsDestroy",
              "cuvsTieredIndexBuild", "cuvsTieredIndexSearch", "cuvsTieredIndexExtend", "cuvsTieredIndexMerge",
              "cuvsAmdTieredIndexGetInfo", "cuvsAmdTieredIndexCompact", "cuvsAmdTieredIndexSearchTiers",
              "cuvsAmdTieredTailSearch", "cuvsAmdTieredMerge", "cuvsAmdTieredCounters"):
        assert hasattr(lib, s), s
    p = C.POINTER(T._CIndexParams)()
    assert lib.cuvsTieredIndexParamsCreate(C.byref(p)) == 1
    v = p.contents
    # c/src/neighbors/tiered_index.cpp:314-324 over cpp/include/cuvs/neighbors/tiered_index.hpp:62-66
    assert (v.metric, v.algo, v.min_ann_rows, v.create_ann_index_on_extend, v.cagra_params, v.ivf_flat_params,
            v.ivf_pq_params) == (0, 0, 100000, False, None, None, None)
    assert lib.cuvsTieredIndexParamsDestroy(p) == 1
    idx = C.POINTER(T._CIndex)()
    assert lib.cuvsTieredIndexCreate(C.byref(idx)) == 1
    assert (idx.contents.addr, idx.contents.algo) == (0, 0)
    size = C.c_int64(0)
    assert lib.cuvsAmdTieredIndexGetInfo(idx, C.byref(size), None, None, None) == 0  # not built: CUVS_ERROR
    lib.cuvsGetLastErrorText.restype = C.c_char_p
    assert b"not built" in lib.cuvsGetLastErrorText()
    assert lib.cuvsTieredIndexDestroy(idx) == 1


def test_python_index_params_properties():
    from cuvs_amd.neighbors import ivf_flat, tiered_index as T

    p = T.IndexParams()
    assert (p.metric, p.algo, p.min_ann_rows, p.create_ann_index_on_extend, p.upstream_params) == ("sqeuclidean", "cagra", 100000,
                                                                                                 False, None)
    up = ivf_flat.IndexParams(n_lists=8)
    p = T.IndexParams(metric="inner_product", algo="ivf_flat", upstream_params=up, min_ann_rows=7, create_ann_index_on_extend=True)
    assert (p.metric, p.algo, p.min_ann_rows, p.create_ann_index_on_extend) == ("inner_product", "ivf_flat", 7, True)
    assert p.upstream_params is up and p._p.contents.ivf_flat_params == C.cast(up._p, C.c_void_p).value
    assert p._p.contents.cagra_params is None and p._p.contents.ivf_pq_params is None
    with pytest.raises(TypeError):
        T.IndexParams(algo="cagra", upstream_params=up)
    with pytest.raises(ValueError):
        T.IndexParams(algo="hnsw")
    assert not T.Index().trained


# ---------------------------------------------------------------- the merge rule
def _plain_merge(ad, ai, bd, bi, ann_rows, select_min):
    """The rule in the most literal form: collect the real entries, sort tuples, pad."""
    m, k = ai.shape
    out_d = np.full((m, k), R.worst(select_min), np.float32)
    out_i = np.full((m, k), R.I64_MAX, np.int64)
    for r in range(m):
        ent = [(float(ad[r, j]), int(ai[r, j])) for j in range(k) if 0 <= ai[r, j] < ann_rows]
        ent += [(float(bd[r, j]), int(bi[r, j])) for j in range(bi.shape[1]) if 0 <= bi[r, j] != R.I64_MAX]
        ent.sort(key=lambda e: (e[0] if select_min else -e[0], e[1]))
        for j, (d, i) in enumerate(ent[:k]):
            out_d[r, j], out_i[r, j] = d, i
    return out_d, out_i


def _crafted(k, kb, ann_rows, n_tail, seed, select_min, pad_a, pad_b, ties):
    rng = np.random.default_rng(seed)
    m = 6
    ai = np.stack([rng.choice(ann_rows, size=k, replace=False) for _ in range(m)]).astype(np.int64)
    bi = np.stack([ann_rows + rng.choice(n_tail, size=kb, replace=False) for _ in range(m)]).astype(np.int64)
    if ties:  # a handful of values, so that ties fall inside and across the tiers
        ad = rng.integers(0, 4, size=(m, k)).astype(np.float32)
        bd = rng.integers(0, 4, size=(m, kb)).astype(np.float32)
    else:
        ad = rng.normal(size=(m, k)).astype(np.float32)
        bd = rng.normal(size=(m, kb)).astype(np.float32)
    order = np.argsort(ad if select_min else -ad, axis=1, kind="stable")
    ad, ai = np.take_along_axis(ad, order, 1), np.take_along_axis(ai, order, 1)
    pads = [-1, ann_rows, ann_rows + 5, R.I64_MAX, 0xFFFFFFFF]  # the forms an ANN tier's missing slot takes
    for r in range(m):
        pos = {"none": [], "last": [k - 1], "half": list(range(k // 2, k)), "all": list(range(k)), "middle": [k // 2]}[pad_a]
        for j in pos:
            ai[r, j] = pads[(r + j) % len(pads)]
            ad[r, j] = [0.0, -5.0, np.float32(R.F32_MAX), np.float32(-R.F32_MAX)][(r + j) % 4]  # distance says nothing
        for j in ({"none": [], "last": [kb - 1], "all": list(range(kb))}[pad_b]):
            bi[r, j] = R.I64_MAX
            bd[r, j] = R.worst(select_min)
    return ad, ai, bd, bi


@pytest.mark.parametrize("select_min", [True, False])
@pytest.mark.parametrize("pad_a", ["none", "last", "half", "all", "middle"])
@pytest.mark.parametrize("pad_b", ["none", "last", "all"])
@pytest.mark.parametrize("k,kb", [(1, 1), (10, 10), (5, 37), (16, 3)])
@pytest.mark.parametrize("ties", [False, True])
def test_merge_restatement_equals_a_plain_sort(k, kb, ties, pad_b, pad_a, select_min):
    ann_rows, n_tail = 0xFFFFFFFF + 10 if k == 5 else 100, 50
    if k == 5:  # 0xffffffff is a real id only when the ANN tier is that large
        ann_rows = 100
    ad, ai, bd, bi = _crafted(k, kb, ann_rows, n_tail, 7 * k + kb, select_min, pad_a, pad_b, ties)
    got_d, got_i = R.merge((ad, ai), (bd, bi), ann_rows, select_min)
    want_d, want_i = _plain_merge(ad, ai, bd, bi, ann_rows, select_min)
    assert (got_i == want_i).all()
    assert (got_d.view(np.uint32) == want_d.view(np.uint32)).all()
    real = (got_i != R.I64_MAX)
    assert (got_d[~real] == R.worst(select_min)).all()
    # real entries first, in order; on a tie the ANN entry (the smaller id) stands first
    for r in range(got_i.shape[0]):
        n_real = int(real[r].sum())
        assert real[r, :n_real].all()
        key = got_d[r, :n_real] if select_min else -got_d[r, :n_real]
        assert all((key[j], got_i[r, j]) < (key[j + 1], got_i[r, j + 1]) for j in range(n_real - 1))
    total = ((ai >= 0) & (ai < ann_rows)).sum(1) + (bi != R.I64_MAX).sum(1)
    assert (real.sum(1) == np.minimum(total, k)).all()


def test_merge_keeps_ann_entries_on_ties_and_ignores_padding_distances():
    ai = np.array([[3, 7, -1]], np.int64)
    ad = np.array([[1.0, 2.0, -9.0]], np.float32)  # the padding slot's distance would win if it were looked at
    bi = np.array([[100, 101, R.I64_MAX]], np.int64)
    bd = np.array([[1.0, 2.0, 0.0]], np.float32)
    d, i = R.merge((ad, ai), (bd, bi), 100)
    assert i.tolist() == [[3, 100, 7]] and d.tolist() == [[1.0, 1.0, 2.0]]
    d, i = R.merge((ad, ai), (bd, bi), 100, select_min=False)
    assert i.tolist() == [[7, 101, 3]] and d.tolist() == [[2.0, 2.0, 1.0]]
    d, i = R.merge((ad[:, :1], np.array([[R.I64_MAX]])), (bd[:, 2:], bi[:, 2:]), 100, select_min=False)
    assert i.tolist() == [[R.I64_MAX]] and d[0, 0] == -R.F32_MAX


def test_globalize_and_tail_bits():
    d = np.array([[0.5, 2.0, R.F32_MAX, R.F32_MAX]], np.float32)
    i = np.array([[4, 1, 0, -1]], np.int64)  # row 0 was filtered (worst value), the last slot is missing
    gd, gi = R.globalize(d, i, 600)
    assert gi.tolist() == [[604, 601, R.I64_MAX, R.I64_MAX]] and gd[0, 2] == R.F32_MAX
    rng = np.random.default_rng(3)
    for ann_rows, n_tail in [(0, 5), (37, 70), (64, 1), (95, 33)]:
        keep = rng.random(ann_rows + n_tail) < 0.4
        words = R.tail_bits(R.pack_bits(keep), ann_rows, n_tail)
        got = [(int(words[j >> 5]) >> (j & 31)) & 1 for j in range(n_tail)]
        assert got == keep[ann_rows:].astype(int).tolist()
        assert len(words) == (n_tail + 31) // 32 and (int(words[-1]) >> ((n_tail - 1) % 32 + 1)) == 0


def test_growth_policy():
    assert [R.initial_capacity(n) for n in (0, 1, 15, 16, 500, 600, 100000)] == [0, 1, 15, 17, 531, 637, 106250]
    # the walk of the GPU test: 600 rows, then 1, 1, 1, 130, 40
    cap, size, caps = R.initial_capacity(600), 600, []
    for new in (1, 1, 1, 130, 40):
        cap = R.grown_capacity(size, cap, new)
        size += new
        caps.append(cap)
    assert caps == [637, 637, 637, 1274, 1274]
    assert R.grown_capacity(637, 637, 0) == 637          # exact fit: nothing moves
    assert R.grown_capacity(600, 637, 37) == 637         # exact fit with rows
    assert R.grown_capacity(600, 637, 38) == 1274        # one row too many: doubling
    assert R.grown_capacity(600, 637, 5000) == 5600      # more than double: what is needed
    assert R.grown_capacity(0, 0, 3) == 3
    assert not R.builds_ann(500, 500) and R.builds_ann(501, 500)

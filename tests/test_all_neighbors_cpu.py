"""CPU: ABI layout of include/cuvs/neighbors/all_neighbors.h, the reference's C driver against our headers, and the numpy
restatement (tests/all_neighbors_ref.py) against a slow set-based merge."""
import os
import subprocess

import numpy as np
import pytest

from tests import all_neighbors_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")

_PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include <cuvs/core/all.h>
#include <cuvs_amd/extensions.h>
int main(void) {
  printf("sizeof %zu\n", sizeof(struct cuvsAllNeighborsIndexParams));
  printf("algo %zu\n", offsetof(struct cuvsAllNeighborsIndexParams, algo));
  printf("overlap_factor %zu\n", offsetof(struct cuvsAllNeighborsIndexParams, overlap_factor));
  printf("n_clusters %zu\n", offsetof(struct cuvsAllNeighborsIndexParams, n_clusters));
  printf("metric %zu\n", offsetof(struct cuvsAllNeighborsIndexParams, metric));
  printf("ivf_pq_params %zu\n", offsetof(struct cuvsAllNeighborsIndexParams, ivf_pq_params));
  printf("nn_descent_params %zu\n", offsetof(struct cuvsAllNeighborsIndexParams, nn_descent_params));
  printf("enum %d %d %d\n", (int)CUVS_ALL_NEIGHBORS_ALGO_BRUTE_FORCE, (int)CUVS_ALL_NEIGHBORS_ALGO_IVF_PQ,
         (int)CUVS_ALL_NEIGHBORS_ALGO_NN_DESCENT);
  return 0;
}
"""


def test_struct_layout_and_enum_values(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(_PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-I", INC, str(src), "-o", str(exe)])
    got = subprocess.check_output([str(exe)]).decode().split("\n")
    assert got[:8] == ["sizeof 48", "algo 0", "overlap_factor 8", "n_clusters 16", "metric 24", "ivf_pq_params 32",
                       "nn_descent_params 40", "enum 0 1 2"]


def test_params_create_defaults_and_destroy_with_nested():
    import ctypes as C

    from cuvs_amd.neighbors.all_neighbors import _CParams

    lib = C.CDLL(os.path.join(ROOT, "cuvs_amd", "libcuvs_c.so"))
    p = C.POINTER(_CParams)()
    assert lib.cuvsAllNeighborsIndexParamsCreate(C.byref(p)) == 1
    c = p.contents
    assert (c.algo, c.overlap_factor, c.n_clusters, c.metric) == (0, 1, 1, 0)
    assert c.ivf_pq_params is None and c.nn_descent_params is None
    pq, nnd = C.c_void_p(), C.c_void_p()
    assert lib.cuvsIvfPqIndexParamsCreate(C.byref(pq)) == 1 and lib.cuvsNNDescentIndexParamsCreate(C.byref(nnd)) == 1
    c.ivf_pq_params, c.nn_descent_params = pq.value, nnd.value
    assert lib.cuvsAllNeighborsIndexParamsDestroy(p) == 1  # frees both nested structs too
    assert lib.cuvsAllNeighborsIndexParamsDestroy(None) == 1


def test_reference_c_driver_compiles_and_links(tmp_path):
    """c/tests/neighbors/run_all_neighbors_c.c compiles unchanged against include/ and links against libcuvs_c.so with no
    unresolved symbol. Needs the reference tree, which only exists in the build container."""
    drv = "/root/reference/c/tests/neighbors/run_all_neighbors_c.c"
    if not os.path.exists(drv):
        pytest.skip("no reference tree on this machine")
    so = tmp_path / "driver.so"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror=implicit-function-declaration", "-fPIC", "-shared", "-I", INC, drv,
                           "-L", os.path.join(ROOT, "cuvs_amd"), "-lcuvs_c", "-Wl,--no-undefined", "-o", str(so)])
    assert so.exists()


def _random_merge_case(rng, n, m, k, select_min, filled):
    """A global matrix with `filled` valid columns per row (sorted, distinct ids) and a batch over a random inverted list;
    distances from a small set so that equal distances with different ids abound, batch entries partly duplicating the
    global ones (same id, same distance)."""
    fid, fd = R.fill_values(select_min)
    sign = 1.0 if select_min else -1.0
    dist_of = lambda a, b: np.float32(sign * (1 + (a * 7 + b * 13) % 5) * 0.25)  # a function of the PAIR: one value wherever it is computed
    inv = np.sort(rng.choice(n, m, replace=False)).astype(np.int64)
    gi = np.full((n, k), fid, np.int64)
    gd = np.full((n, k), fd, np.float32)
    for g in range(n):
        f = int(filled[g])
        ids = rng.choice(n, f, replace=False)
        ent = sorted((sign * float(dist_of(min(g, j), max(g, j))), int(j)) for j in ids)
        for c, (d, j) in enumerate(ent):
            gi[g, c], gd[g, c] = j, np.float32(sign * d)
    bi = np.empty((m, k), np.int64)
    bd = np.empty((m, k), np.float32)
    for b in range(m):
        loc = rng.choice(m, min(k, m), replace=False)
        ent = sorted((sign * float(dist_of(min(inv[b], inv[l]), max(inv[b], inv[l]))), int(l)) for l in loc)
        row_i = [l for _, l in ent] + [-1] * (k - len(ent))
        row_d = [np.float32(sign * d) for d, _ in ent] + [fd] * (k - len(ent))
        bi[b], bd[b] = row_i, row_d
    return inv, bi, bd, gi, gd


@pytest.mark.parametrize("select_min", [True, False])
@pytest.mark.parametrize("k", [1, 3, 8])
def test_restatement_merge_equals_set_based_merge(k, select_min):
    rng = np.random.default_rng(100 + k)
    n, m = 40, 25
    filled = rng.integers(0, k + 1, n)  # unfilled, partly filled and full rows
    inv, bi, bd, gi, gd = _random_merge_case(rng, n, m, k, select_min, filled)
    want_i, want_d = R.slow_merge(inv, bi, bd, gi, gd, select_min)
    got_i, got_d = R.remap_merge(inv, bi, bd, gi.copy(), gd.copy(), select_min)
    assert (got_i == want_i).all() and (got_d.view(np.uint32) == want_d.view(np.uint32)).all()
    fid, _ = R.fill_values(select_min)
    for g in range(n):
        real = got_i[g][got_i[g] != fid]
        assert len(set(real.tolist())) == len(real)  # no id twice
        key = R.float_key(got_d[g] if select_min else -got_d[g]).astype(np.int64)
        assert (np.diff(key) >= 0).all()
    untouched = np.setdiff1d(np.arange(n), inv)
    assert (got_i[untouched] == gi[untouched]).all() and (got_d[untouched] == gd[untouched]).all()


def test_restatement_merge_drops_a_repeated_id_even_at_a_different_distance():
    inv = np.array([0, 1, 2], np.int64)
    gi = np.array([[1, 2], [0, 2], [0, 1]], np.int64)
    gd = np.array([[1.0, 2.0], [1.0, 3.0], [2.0, 3.0]], np.float32)
    bi = np.array([[2, 1], [0, 2], [1, 0]], np.int64)
    bd = np.array([[0.5, 1.0], [1.0, 3.0], [3.0, 4.0]], np.float32)  # row 0 sees id 2 at 0.5 AND (globally) at 2.0
    R.remap_merge(inv, bi, bd, gi, gd)
    assert gi[0].tolist() == [2, 1] and gd[0].tolist() == [0.5, 1.0]
    assert gi[2].tolist() == [0, 1] and gd[2].tolist() == [2.0, 3.0]


def test_inverted_lists_shift_and_reachability():
    nearest = np.array([[0, 2], [1, 0], [2, 1], [0, 1]], np.int64)
    inv, sizes, offsets = R.inverted_lists(nearest, 3)
    assert sizes.tolist() == [3, 3, 2] and offsets.tolist() == [0, 3, 6]
    assert inv.tolist() == [0, 1, 3, 1, 2, 3, 0, 2]
    ids = np.array([[5, 6, 7], [8, 9, 10]], np.int64)
    d = np.array([[1, 2, 3], [4, 5, 6]], np.float32)
    si, sd = R.shift(ids, d)
    assert si.tolist() == [[0, 5, 6], [1, 8, 9]] and sd.tolist() == [[0, 1, 2], [0, 4, 5]]
    _, sd = R.shift(ids, d, first=np.array([9, 8], np.float32))
    assert sd[:, 0].tolist() == [9, 8]
    core = np.array([1.0, 4.0], np.float32)
    out = R.reach_epilogue(np.array([[0.0, 6.0], [6.0, 0.0]], np.float32), core, core, 0.5)
    assert out.tolist() == [[1.0, 4.0], [4.0, 4.0]]
    assert R.core_distances(d).tolist() == [3.0, 6.0]

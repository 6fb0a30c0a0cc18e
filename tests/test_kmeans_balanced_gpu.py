"""GPU: the balanced k-means trainer (cuvs_amd/csrc/kmeans_balanced.hip) through its step hooks - cluster means on constructed
labels (every packing of cluster_means_kernel, the unrolled row loop and its tail, dims above 64), group_by_label on its own,
build_clusters with a row pitch and in-row offset, one adjust_centers pass on a constructed state, and balanced_fit down every
host-side branch - for L2 and inner product.

Two kinds of assertion: T, bit for bit against the twin (oracle/oracle_kmeans.c), and R, against float64 numpy or an invariant
(tests/kmeans_balanced_ref.py), which a mistake shared with the twin cannot pass. The cases, their data and the twin's results
are shared with tests/test_kmeans_balanced_cpu.py, which also proves that each shape reaches its branch."""
import ctypes as C

import numpy as np
import pytest

from tests import kmeans_balanced_ref as K

pytestmark = pytest.mark.gpu


class _Gpu:
    """The cuvsAmd* step hooks on torch tensors; a pitched input is a view `buf[:, col0:col0 + dim]` of a device matrix."""

    def __init__(self):
        import torch
        import cuvs_amd
        from cuvs_amd._lib import check, lib

        self.torch, self.check, self.lib = torch, check, lib()
        self.res = cuvs_amd.common.Resources()

    def dev(self, a):
        return self.torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the shared inputs are read-only

    def empty(self, shape, dtype):
        return self.torch.empty(shape, dtype=dtype, device="cuda")

    def rows(self, buf, col0):
        t = self.dev(buf)
        return t, t.data_ptr() + 4 * col0, buf.shape[0], buf.shape[1]

    def call(self, name, argtypes, *args):
        fn = getattr(self.lib, name)
        fn.argtypes = argtypes
        self.check(fn(self.res.get_c_obj(), *args))
        self.res.sync()

    @staticmethod
    def u32(t):
        return t.cpu().numpy().view(np.uint32)

    def cluster_means(self, buf, col0, dim, labels, k):
        t, px, n, ld = self.rows(buf, col0)
        lab = self.dev(labels.view(np.int32))
        centers, sizes = self.empty((k, dim), self.torch.float32), self.empty((k,), self.torch.int32)
        self.call("cuvsAmdKMeansClusterMeans",
                  [C.c_size_t, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
                  px, n, ld, dim, k, lab.data_ptr(), centers.data_ptr(), sizes.data_ptr())
        return centers.cpu().numpy(), self.u32(sizes)

    def group_by_label(self, labels, k):
        n = len(labels)
        lab = self.dev(labels.view(np.int32))
        perm, offsets = self.empty((n,), self.torch.int32), self.empty((k + 1,), self.torch.int32)
        self.call("cuvsAmdGroupByLabel", [C.c_size_t, C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p],
                  lab.data_ptr(), n, k, perm.data_ptr(), offsets.data_ptr())
        return self.u32(perm), self.u32(offsets)

    def build_clusters(self, buf, col0, dim, k, n_iters, inner_product):
        t, px, n, ld = self.rows(buf, col0)
        centers = self.empty((k, dim), self.torch.float32)
        labels, sizes = self.empty((n,), self.torch.int32), self.empty((k,), self.torch.int32)
        self.call("cuvsAmdKMeansBuildClusters",
                  [C.c_size_t, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                   C.c_void_p],
                  px, n, ld, dim, k, n_iters, int(inner_product), centers.data_ptr(), labels.data_ptr(), sizes.data_ptr())
        return centers.cpu().numpy(), self.u32(labels), self.u32(sizes)

    def adjust_centers(self, centers, buf, col0, dim, labels, sizes, threshold, i_primes):
        t, px, n, ld = self.rows(buf, col0)
        c, lab, sz = self.dev(centers), self.dev(labels.view(np.int32)), self.dev(sizes.view(np.int32))
        ip, adjusted = C.c_int(i_primes), C.c_int(-1)
        self.call("cuvsAmdKMeansAdjustCenters",
                  [C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_float,
                   C.POINTER(C.c_int), C.POINTER(C.c_int)],
                  c.data_ptr(), centers.shape[0], dim, px, ld, n, lab.data_ptr(), sz.data_ptr(), threshold, C.byref(ip),
                  C.byref(adjusted))
        return c.cpu().numpy(), adjusted.value, ip.value

    def balanced_fit(self, x, k, n_iters, hierarchical, inner_product):
        t = self.dev(x)
        n, dim = x.shape
        centers, labels = self.empty((k, dim), self.torch.float32), self.empty((n,), self.torch.int32)
        self.call("cuvsAmdKMeansBalancedFitEx",
                  [C.c_size_t, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p],
                  t.data_ptr(), n, dim, k, n_iters, int(hierarchical), int(inner_product), centers.data_ptr(),
                  labels.data_ptr())
        return centers.cpu().numpy(), self.u32(labels)


@pytest.fixture(scope="module")
def gpu():
    return _Gpu()


def _same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.tobytes() != want.tobytes():
        diff = np.flatnonzero(got.ravel().view(np.uint32) != want.ravel().view(np.uint32))
        raise AssertionError(f"{what}: {len(diff)} of {got.size} differ from the twin, first at {diff[0]}: "
                             f"{got.ravel()[diff[0]]!r} != {want.ravel()[diff[0]]!r}")


# ---------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("pitch", K.MEANS_PITCHES)
@pytest.mark.parametrize("dim", K.MEANS_DIMS)
def test_cluster_means_on_constructed_labels(gpu, dim, pitch):
    x, labels, k = K.means_case(dim)
    buf, col0 = K.means_buf(dim, pitch)
    centers, sizes = gpu.cluster_means(buf, col0, dim, labels, k)
    worst = K.check_means(x, labels, k, centers, sizes)                      # R
    print(f"dim {dim} {pitch}: worst ratio to the summation bound {worst:.3f}")
    want_c, want_s = K.twin_means(dim, pitch)                                # T
    assert (sizes == want_s).all()
    _same_bits(centers, want_c, "centres")


# ---------------------------------------------------------------------------------------------- B
def _uniform(n, k):
    return np.random.default_rng(n + k).integers(0, k, n).astype(np.uint32)


GROUP_CASES = {
    "1-1": lambda: (np.zeros(1, np.uint32), 1),
    "1000-1": lambda: (np.zeros(1000, np.uint32), 1),
    "5000-2": lambda: (_uniform(5000, 2), 2),
    "5000-1000": lambda: (_uniform(5000, 1000), 1000),
    "5000-1024": lambda: (_uniform(5000, 1024), 1024),     # one full chunk of the scan
    "5000-1025": lambda: (_uniform(5000, 1025), 1025),     # the carry into a second chunk; 11 key bits
    "5000-2049": lambda: (_uniform(5000, 2049), 2049),
    "200000-70001": lambda: (_uniform(200000, 70001), 70001),
    "3000-3001-ends": lambda: (np.random.default_rng(7).choice(np.array([0, 3000], np.uint32), 3000), 3001),
    "4096-64-one": lambda: (np.full(4096, 37, np.uint32), 64),
}


@pytest.mark.parametrize("case", list(GROUP_CASES))
def test_group_by_label(gpu, case):
    labels, k = GROUP_CASES[case]()
    perm, offsets = gpu.group_by_label(labels, k)
    assert (perm == np.argsort(labels, kind="stable")).all()
    want = np.concatenate([[0], np.cumsum(np.bincount(labels, minlength=k))])
    assert offsets.shape == want.shape and (offsets == want).all()


# ---------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("inner_product", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("case", range(len(K.BUILD_CASES)))
def test_build_clusters(gpu, case, inner_product):
    n, ld, col0, dim, k, skew = K.BUILD_CASES[case]
    x, buf, _ = K.build_case(case, inner_product)
    centers, labels, sizes = gpu.build_clusters(buf, col0, dim, k, K.BUILD_ITERS, inner_product)
    assert (labels < k).all()
    worst = K.check_means(x, labels, k, centers, sizes)                      # R: sizes, zero centres, the bound of A
    print(f"case {K.BUILD_CASES[case]}: worst ratio to the summation bound {worst:.3f}, {(sizes == 0).sum()} empty")
    if n == 701:
        assert (sizes == 0).any()   # clusters that stay empty to the end; check_means has seen their centres to be zero
    want_c, want_l, want_s, _ = K.twin_build(case, inner_product)            # T
    assert (sizes == want_s).all(), f"{(sizes != want_s).sum()} sizes differ from the twin"
    assert (labels == want_l).all(), f"{(labels != want_l).sum()} labels differ from the twin"
    _same_bits(centers, want_c, "centres")


# ---------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("case", range(len(K.ADJUST_CASES)))
def test_adjust_centers_pass(gpu, case):
    n, dim, ld, col0, threshold, ip0, _ = K.ADJUST_CASES[case]
    _, buf, labels, sizes, centers = K.adjust_case(case)
    new_centers, adjusted, i_primes = gpu.adjust_centers(centers, buf, col0, dim, labels, sizes, threshold, ip0)
    K.check_adjust(case, new_centers, adjusted, i_primes)                    # R
    want_c, want_a, want_ip = K.twin_adjust(case)                            # T
    assert (adjusted, i_primes) == (want_a, want_ip)
    _same_bits(new_centers, want_c, "centres")


# ---------------------------------------------------------------------------------------------- E
@pytest.mark.parametrize("inner_product", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("case", range(len(K.FIT_CASES)))
def test_balanced_fit(gpu, case, inner_product):
    n, dim, k, hier, skew = K.FIT_CASES[case]
    x = K.fit_case(case, inner_product)
    centers, labels = gpu.balanced_fit(x, k, K.FIT_ITERS, hier, inner_product)
    worst = K.check_assignment(x, centers, labels, inner_product)            # R
    print(f"case {K.FIT_CASES[case]}: worst ratio of a label's gap to its rounding bound {worst:.3f}")
    want_c, want_l, _ = K.twin_fit(case, inner_product)                      # T
    _same_bits(centers, want_c, "centres")
    assert (labels == want_l).all(), f"{(labels != want_l).sum()} labels differ from the twin"

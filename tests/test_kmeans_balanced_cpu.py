"""CPU: the twin of the balanced k-means (oracle/oracle_kmeans.c) against float64 numpy, and the trace counters that prove
every shape of tests/kmeans_balanced_ref.py reaches the branch it is there for. tests/test_kmeans_balanced_gpu.py compares the
HIP code with this twin bit for bit; the checks here are the ones a mistake shared by both could not pass."""
import pytest

import oracle
from tests import kmeans_balanced_ref as K

SKEW_BUILD = [i for i, c in enumerate(K.BUILD_CASES) if c[5]]
SKEW_FIT = [i for i, c in enumerate(K.FIT_CASES) if c[4]]


@pytest.mark.parametrize("pitch", K.MEANS_PITCHES)
@pytest.mark.parametrize("dim", K.MEANS_DIMS)
def test_cluster_means_within_summation_bound(dim, pitch):
    x, labels, k = K.means_case(dim)
    centers, sizes = K.twin_means(dim, pitch)
    worst = K.check_means(x, labels, k, centers, sizes)
    print(f"dim {dim} {pitch}: worst ratio to the bound {worst:.3f}")
    # the pitch changes addresses only
    dense = K.twin_means(dim, "dense")
    assert centers.tobytes() == dense[0].tobytes() and (sizes == dense[1]).all()


@pytest.mark.parametrize("inner_product", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("case", range(len(K.BUILD_CASES)))
def test_build_clusters_invariants(case, inner_product):
    n, ld, col0, dim, k, skew = K.BUILD_CASES[case]
    x, _, _ = K.build_case(case, inner_product)
    centers, labels, sizes, trace = K.twin_build(case, inner_product)
    worst = K.check_means(x, labels, k, centers, sizes)
    print(f"case {K.BUILD_CASES[case]}: worst ratio {worst:.3f}, trace {trace}")
    assert trace["empty_at_return"] == int((sizes == 0).sum())
    if n == 6177:
        assert trace["primes_skipped"] > 0
    if skew:
        assert trace["adjust_passes"] > 0 and trace["extra_iters"] > 0
    if n == 701:
        assert trace["empty_at_return"] > 0  # check_means has seen their centres to be zero


@pytest.mark.parametrize("case", range(len(K.ADJUST_CASES)))
def test_adjust_centers_pass(case):
    new_centers, adjusted, i_primes = K.twin_adjust(case)
    K.check_adjust(case, new_centers, adjusted, i_primes)


@pytest.mark.parametrize("inner_product", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("case", range(len(K.FIT_CASES)))
def test_balanced_fit_invariants(case, inner_product):
    n, dim, k, hier, skew = K.FIT_CASES[case]
    x = K.fit_case(case, inner_product)
    centers, labels, trace = K.twin_fit(case, inner_product)
    worst = K.check_assignment(x, centers, labels, inner_product)
    print(f"case {K.FIT_CASES[case]}: worst ratio {worst:.3f}, trace {trace}")
    if skew:
        assert trace["adjust_passes"] > 0 and trace["extra_iters"] > 0
    if (n, dim, k) == (6000, 96, 300):
        assert trace["meso_truncated"] > 0
    if (n, dim, k) == (300, 16, 256):
        assert trace["meso_cyclic"] > 0 and trace["empty_at_return"] > 0
    assert trace["flat_route"] == (1 if k <= 2 or not hier else 0)


@pytest.mark.parametrize("case", [i for i, c in enumerate(K.FIT_CASES) if c[2] > 1])
def test_inner_product_flag_changes_the_labels(case):
    """On the log-normal-scaled rows the nearest centre and the centre of the largest dot product differ for some row."""
    _, l2_labels, _ = K.twin_fit(case, False, lognormal=True)
    _, ip_labels, _ = K.twin_fit(case, True)
    assert (l2_labels != ip_labels).any()


def test_defaults_are_the_l2_run():
    x = K.fit_case(3, False)
    c0, l0 = oracle.kmeans_balanced_fit(x, 3, K.FIT_ITERS, True)
    c1, l1, _ = K.twin_fit(3, False)
    assert c0.tobytes() == c1.tobytes() and (l0 == l1).all()


def test_earlier_c_entry_points_keep_their_arguments():
    """oracle_kmeans_balanced_fit / oracle_kmeans_build_clusters without metric and trace: the L2 run, as before."""
    import ctypes as C

    import numpy as np

    x = np.array(K.fit_case(3, False))
    n, dim = x.shape
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    centers, labels = np.empty((3, dim), np.float32), np.empty(n, np.uint32)
    oracle.lib().oracle_kmeans_balanced_fit(p(x), C.c_int64(n), C.c_int(dim), C.c_int(3), C.c_int(K.FIT_ITERS), C.c_int(1),
                                            p(centers), p(labels))
    want_c, want_l, _ = K.twin_fit(3, False)
    assert centers.tobytes() == want_c.tobytes() and (labels == want_l).all()
    sizes = np.empty(3, np.uint32)
    oracle.lib().oracle_kmeans_build_clusters(p(x), C.c_int64(n), C.c_int64(dim), C.c_int(dim), C.c_int(3),
                                              C.c_int(K.BUILD_ITERS), p(centers), p(labels), p(sizes))
    want = oracle.kmeans_build_clusters(x, 3, K.BUILD_ITERS)
    assert centers.tobytes() == want[0].tobytes() and (labels == want[1]).all() and (sizes == want[2]).all()

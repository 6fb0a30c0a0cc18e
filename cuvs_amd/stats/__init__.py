"""cuvs.stats: silhouette score and trustworthiness on the device (reference: cpp/include/cuvs/stats/silhouette_score.hpp and
trustworthiness_score.hpp, which have no C or Python layer; C entry points: include/cuvs_amd/stats.h, contract: DESIGN.md 3.1y).

X, X_embedded, labels and neighbors are torch tensors on the device (fp32 rows, int32 labels, int64 neighbour ids), row-major and
contiguous; they are handed to the library as they are, which refuses anything else."""
import ctypes as C

import torch

from .._lib import Tensor, check, lib
from ..common import auto_sync_resources
from ..distance import DISTANCE_TYPES
from ..neighbors._util import optional_tensor as _t

METRICS = dict(DISTANCE_TYPES, manhattan=3)


def _metric(metric):
    return METRICS[metric] if isinstance(metric, str) else int(metric)


def _n_labels(labels, n_unique_labels):
    return int(labels.max().item()) + 1 if n_unique_labels is None else int(n_unique_labels)


def _silhouette(X, labels, n_unique_labels, metric, batch_size, scores, resources):
    tx, tl = Tensor(X), Tensor(labels)
    ts, ps = _t(scores)
    mean = C.c_double(float("nan"))
    check(lib().cuvsAmdSilhouetteScore(resources.get_c_obj(), tx.ptr, tl.ptr, C.c_int64(_n_labels(labels, n_unique_labels)),
                                       C.c_int(_metric(metric)), C.c_int64(batch_size or 0), ps, C.byref(mean)))
    return mean.value


@auto_sync_resources
def silhouette_score(X, labels, n_unique_labels=None, metric="sqeuclidean", batch_size=None, scores=None, resources=None):
    """Mean silhouette coefficient of all samples. `batch_size` caps the rows processed at a time (the reference's
    silhouette_score_batched chunk); the result is bit-identical for every value. `scores` (fp32 [n]), when given, receives the
    per-sample coefficients. `n_unique_labels=None` takes labels.max() + 1."""
    return _silhouette(X, labels, n_unique_labels, metric, batch_size, scores, resources)


@auto_sync_resources
def silhouette_samples(X, labels, n_unique_labels=None, metric="sqeuclidean", batch_size=None, resources=None):
    """The silhouette coefficient of every sample, fp32 [n] on the device."""
    scores = torch.empty(X.shape[0], dtype=torch.float32, device=X.device)
    _silhouette(X, labels, n_unique_labels, metric, batch_size, scores, resources)
    return scores


@auto_sync_resources
def neighbor_ranks(X, neighbors, ranks=None, resources=None):
    """(ranks int32 [n, k], penalty_sum): the 1-based rank of neighbors[i][q] among the other rows of X by squared L2 distance
    from row i (ties to the smaller index), and the sum of max(0, rank - k). `ranks=False` leaves the matrix out (None is
    returned in its place)."""
    if ranks is None:
        ranks = torch.empty(tuple(neighbors.shape), dtype=torch.int32, device=X.device)
    elif ranks is False:
        ranks = None
    tx, tn = Tensor(X), Tensor(neighbors)
    tr, pr = _t(ranks)
    penalty = C.c_uint64(0)
    check(lib().cuvsAmdNeighborRanks(resources.get_c_obj(), tx.ptr, tn.ptr, pr, C.byref(penalty)))
    return ranks, penalty.value


@auto_sync_resources
def trustworthiness_score(X, X_embedded, n_neighbors=5, metric="euclidean", resources=None):
    """How far the n_neighbors nearest rows of every row of X_embedded are also near it in X (1.0: none is further than rank
    n_neighbors), as sklearn.manifold.trustworthiness. metric: one of the L2 names; the ranks are taken on squared distances."""
    tx, te = Tensor(X), Tensor(X_embedded)
    score = C.c_double(float("nan"))
    check(lib().cuvsAmdTrustworthinessScore(resources.get_c_obj(), tx.ptr, te.ptr, C.c_int64(n_neighbors), C.c_int(_metric(metric)),
                                            C.byref(score)))
    return score.value


def last_stats():
    """Counters of the calling thread's last call: pair tiles, row slabs, and straddling tiles (silhouette) or pairs past the
    screen (ranks)."""
    out = (C.c_uint64 * 4)()
    check(lib().cuvsAmdStatsLastStats(out))
    return dict(tiles=out[0], slabs=out[1], straddling_or_passed=out[2])

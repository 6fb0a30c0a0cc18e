"""Single-linkage agglomerative clustering (reference: cpp/include/cuvs/cluster/agglomerative.hpp - single_linkage,
helpers::build_linkage, helpers::build_dendrogram; C entry points: include/cuvs_amd/single_linkage.h).

X is a torch tensor on the device, fp32, row-major and contiguous; it is handed to the library as it is, which refuses
anything else. Edge weights come from the fp32 chain acc = fmaf(x[i][t] - x[j][t], x[i][t] - x[j][t], acc), t ascending (its
square root for the euclidean metrics), and edges are ordered by (bits of the weight, smaller end, larger end)."""
import ctypes as C

import torch

from .._lib import Tensor, check, lib
from ..common import auto_sync_resources
from ..distance import DISTANCE_TYPES
from ..neighbors._util import optional_tensor as _t
from ..neighbors.all_neighbors import AllNeighborsParams

LINKAGES = {"pairwise": 0, "knn_graph": 1}
SPACES = {"distance": 0, "mutual_reachability": 1}


class _CParams(C.Structure):
    _fields_ = [
        ("space", C.c_int),
        ("c", C.c_int),
        ("linkage", C.c_int),
        ("min_samples", C.c_int),
        ("alpha", C.c_float),
        ("all_neighbors_params", C.c_void_p),
    ]


def _metric(metric):
    return DISTANCE_TYPES[metric] if isinstance(metric, str) else int(metric)


def _linkage(linkage):
    return LINKAGES[linkage] if isinstance(linkage, str) else int(linkage)


@auto_sync_resources
def single_linkage(X, n_clusters, metric="euclidean", linkage="knn_graph", c=15, dtype=torch.int64, dendrogram=None, labels=None,
                   resources=None):
    """Returns (dendrogram [n - 1, 2], labels [n]) of `dtype` (int32 or int64); buffers that are passed are filled."""
    n = X.shape[0]
    if dendrogram is None:
        dendrogram = torch.empty((max(n - 1, 0), 2), dtype=dtype, device=X.device)
    if labels is None:
        labels = torch.empty(n, dtype=dtype, device=X.device)
    tx, td, tl = Tensor(X), Tensor(dendrogram), Tensor(labels)
    check(lib().cuvsAmdSingleLinkage(resources.get_c_obj(), tx.ptr, td.ptr, tl.ptr, C.c_int(_metric(metric)),
                                     C.c_int64(n_clusters), C.c_int(_linkage(linkage)), C.c_int(c)))
    return dendrogram, labels


@auto_sync_resources
def build_linkage(X, metric="euclidean", space="distance", linkage="knn_graph", c=15, min_samples=5, alpha=1.0,
                  all_neighbors_params=None, dtype=torch.int64, outputs=None, resources=None):
    """The spanning tree and its dendrogram. Returns a dict with mst_src, mst_dst (`dtype`), mst_weights (fp32), each [n - 1] in
    ascending order of (bits(w), src, dst) with src < dst; dendrogram [n - 1, 2], out_distances, out_sizes; and core_dists
    (fp32 [n]; None in distance space). `outputs` may hold buffers under those names; a name mapped to False leaves that
    output out."""
    if all_neighbors_params is not None and not isinstance(all_neighbors_params, AllNeighborsParams):
        raise TypeError("all_neighbors_params must be an instance of AllNeighborsParams")
    n = X.shape[0]
    m = max(n - 1, 0)
    space_id = SPACES[space] if isinstance(space, str) else int(space)
    shapes = dict(mst_src=((m,), dtype), mst_dst=((m,), dtype), mst_weights=((m,), torch.float32), dendrogram=((m, 2), dtype),
                  out_distances=((m,), torch.float32), out_sizes=((m,), dtype))
    if space_id == SPACES["mutual_reachability"]:
        shapes["core_dists"] = ((n,), torch.float32)
    out = dict(outputs or {})
    for name, (shape, dt) in shapes.items():
        if out.get(name) is None:
            out[name] = torch.empty(shape, dtype=dt, device=X.device)
        elif out[name] is False:
            out[name] = None
    out.setdefault("core_dists", None)
    p = C.POINTER(_CParams)()
    check(lib().cuvsAmdLinkageParamsCreate(C.byref(p)))
    try:
        p.contents.space = space_id
        p.contents.c = c
        p.contents.linkage = _linkage(linkage)
        p.contents.min_samples = min_samples
        p.contents.alpha = alpha
        p.contents.all_neighbors_params = all_neighbors_params.get_handle() if all_neighbors_params is not None else None
        tx = Tensor(X)
        keep, ptrs = [], []
        for name in ("mst_src", "mst_dst", "mst_weights", "dendrogram", "out_distances", "out_sizes", "core_dists"):
            t, ptr = _t(out[name])
            keep.append(t)
            ptrs.append(ptr)
        check(lib().cuvsAmdBuildLinkage(resources.get_c_obj(), tx.ptr, p, C.c_int(_metric(metric)), *ptrs))
    finally:
        lib().cuvsAmdLinkageParamsDestroy(p)
    return out


@auto_sync_resources
def build_dendrogram(rows, cols, data, dtype=None, resources=None):
    """The dendrogram of a spanning tree whose n - 1 edges (rows, cols, data) are in merge order. Returns (children [n - 1, 2],
    out_delta fp32 [n - 1], out_size [n - 1]); the index outputs have the type of `rows`."""
    m = rows.shape[0]
    dtype = dtype or rows.dtype
    children = torch.empty((m, 2), dtype=dtype, device=rows.device)
    out_delta = torch.empty(m, dtype=torch.float32, device=rows.device)
    out_size = torch.empty(m, dtype=dtype, device=rows.device)
    ts = [Tensor(t) for t in (rows, cols, data, children, out_delta, out_size)]
    check(lib().cuvsAmdBuildDendrogram(resources.get_c_obj(), *[t.ptr for t in ts]))
    return children, out_delta, out_size


def last_stats():
    """Counters of the calling thread's last linkage: k of the kNN graph (0: pairwise), undirected graph edges after
    symmetrising, sparse rounds that joined components, components after the sparse phase, dense rounds, pair tiles."""
    out = (C.c_uint64 * 6)()
    check(lib().cuvsAmdSingleLinkageLastStats(out))
    return dict(k=out[0], graph_edges=out[1], sparse_rounds=out[2], components=out[3], dense_rounds=out[4], tiles=out[5])

"""Masked L2 nearest neighbour and cross-component nearest neighbours (reference: cpp/src/distance/masked_nn.cuh and
cpp/src/sparse/neighbors/cross_component_nn.cuh, which have no C or Python layer; C entry points: include/cuvs_amd/masked_nn.h,
contract: DESIGN.md 3.1zb).

All arguments are torch tensors on the device, row-major and contiguous; they are handed to the library as they are, which
refuses anything else."""
import ctypes as C

import torch

from .._lib import Tensor, check, lib
from ..common import auto_sync_resources
from ..neighbors._util import optional_tensor as _t


@auto_sync_resources
def masked_l2_nn(x, y, adj, group_idxs, *, sqrt=False, out=None, resources=None):
    """(idx int64 [m], dist fp32 [m]): for every row of x (fp32 [m, dim]) the nearest row of y (fp32 [n, dim]) among the groups
    that adj (bool / uint8 [m, G]) switches on for it; group_idxs (int64 [G]) holds the end index of every group of rows of y. A
    row without a candidate gets -1 and FLT_MAX; ties go to the smaller index. `out=(idx, dist)` reduces into the values the two
    tensors hold (results of an earlier call with the same `sqrt`) instead of starting afresh."""
    m = x.shape[0]
    if out is None:
        idx = torch.empty(m, dtype=torch.int64, device=x.device)
        dist = torch.empty(m, dtype=torch.float32, device=x.device)
    else:
        idx, dist = out
    tx, ty, tg, ti, td = Tensor(x), Tensor(y), Tensor(group_idxs), Tensor(idx), Tensor(dist)
    ta, pa = _t(adj)
    check(lib().cuvsAmdMaskedL2NN(resources.get_c_obj(), tx.ptr, ty.ptr, None, None, pa, tg.ptr, C.c_int(bool(sqrt)),
                                  C.c_int(out is None), ti.ptr, td.ptr))
    return idx, dist


@auto_sync_resources
def cross_component_nn(x, colors, n_components=None, *, sqrt=False, out=None, resources=None):
    """For the rows x (fp32 [n, dim]) with component labels colors (int32 [n], any order) returns
    (row_idx int64 [n], row_dist fp32 [n], edge_src int64 [C], edge_dst int64 [C], edge_weight fp32 [C]): every row's nearest
    row of another component, and for every component c the edge with the smallest (weight, src, dst) that leaves it.
    -1 / FLT_MAX stand for "none". `n_components=None` takes colors.max() + 1; `out` may give the five tensors to write."""
    n = x.shape[0]
    if n_components is None:
        n_components = int(colors.max().item()) + 1
    n_components = int(n_components)
    dev = x.device
    if out is None:
        row_idx = torch.empty(n, dtype=torch.int64, device=dev)
        row_dist = torch.empty(n, dtype=torch.float32, device=dev)
        src = torch.empty(max(n_components, 0), dtype=torch.int64, device=dev)
        dst = torch.empty_like(src)
        w = torch.empty(max(n_components, 0), dtype=torch.float32, device=dev)
    else:
        row_idx, row_dist, src, dst, w = out
    ts = [Tensor(t) for t in (x, colors, row_idx, row_dist, src, dst, w)]
    check(lib().cuvsAmdCrossComponentNN(resources.get_c_obj(), ts[0].ptr, ts[1].ptr, C.c_int64(n_components), C.c_int(bool(sqrt)),
                                        ts[2].ptr, ts[3].ptr, ts[4].ptr, ts[5].ptr, ts[6].ptr))
    return row_idx, row_dist, src, dst, w


def masked_nn_last_stats(resources):
    """(pair tiles of the problem, pair tiles computed) of the calling thread's last call on `resources`."""
    out = (C.c_uint64 * 2)()
    check(lib().cuvsAmdMaskedNNLastStats(resources.get_c_obj(), out))
    return out[0], out[1]

"""Exact Hamming kNN and Hamming distance matrices over packed bit codes: uint8 / int8 rows read as bits, such as the output of
cuvs_amd.preprocessing.quantize.binary (C entry points: include/cuvs_amd/binary_knn.h, design: DESIGN.md 3.1zc).

All arguments are torch tensors on the device. Rows may be column slices of a wider buffer (last stride 1); they are handed to
the library as they are, which refuses anything else."""
import ctypes as C

import torch

from .._lib import Tensor, check, lib
from ..common import auto_sync_resources
from ._util import make_filter, out_buffers


@auto_sync_resources
def knn(dataset, queries, k, *, prefilter=None, neighbors=None, distances=None, resources=None):
    """(distances fp32 [m, k], neighbors int64 [m, k]): for every row of queries ([m, nbytes]) the k rows of dataset
    ([n, nbytes], the same dtype) with the smallest (Hamming distance, id). prefilter: None or (uint32 words, BITSET | BITMAP)
    as in brute_force.search. Slots beyond the rows that exist and pass the filter hold FLT_MAX and -1."""
    neighbors, distances = out_buffers(queries.shape[0], k, neighbors, distances)
    flt, keep = make_filter(prefilter)
    td, tq, tn, to = Tensor(dataset), Tensor(queries), Tensor(neighbors), Tensor(distances)
    fn = lib().cuvsAmdBinaryKnn
    fn.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, type(flt)]
    check(fn(resources.get_c_obj(), td.ptr, tq.ptr, tn.ptr, to.ptr, flt))
    del keep
    return distances, neighbors


@auto_sync_resources
def pairwise_distance(x, y, *, out=None, resources=None):
    """fp32 [m, n]: the Hamming distance of every row of x ([m, nbytes]) to every row of y ([n, nbytes])."""
    if out is None:
        out = torch.empty((x.shape[0], y.shape[0]), dtype=torch.float32, device=x.device)
    tx, ty, to = Tensor(x), Tensor(y), Tensor(out)
    check(lib().cuvsAmdBinaryPairwiseDistance(resources.get_c_obj(), tx.ptr, ty.ptr, to.ptr))
    return out


def last_stats(resources):
    """(column splits, fused top-k epilogue ran, 64-byte K chunks per row, query stagings per 256 rows) of the calling thread's
    last knn / pairwise_distance call."""
    out = (C.c_uint64 * 4)()
    check(lib().cuvsAmdBinaryKnnLastStats(resources.get_c_obj(), out))
    return tuple(int(v) for v in out)

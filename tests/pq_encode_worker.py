"""Child process of tests/test_product_quantizer_gpu.py: encodes the shared cases with whatever encoder the environment
selects (CUVS_AMD_PQ_ENCODE=plain behind CUVS_AMD_DEBUG_SWITCHES=1) and writes codes, labels and the encoder launch counters
to an .npz. Usage: python -m tests.pq_encode_worker OUT.npz"""
import ctypes as C
import sys

import numpy as np
import torch

from tests import product_quantizer_ref as P


def encode_case(case, resources=None):
    from cuvs_amd.preprocessing.quantize import pq

    n, pq_dim, pq_len, bits, subspaces, vq = case
    x, book, vq_book = P.make_case(case)
    params = pq.QuantizerParams(pq_bits=bits, pq_dim=pq_dim, use_subspaces=subspaces, use_vq=vq)
    kw = {} if resources is None else {"resources": resources}
    q = pq.from_codebooks(params, torch.from_numpy(book).cuda(), None if vq_book is None else torch.from_numpy(vq_book).cuda(), **kw)
    codes, labels = pq.transform(q, torch.from_numpy(x).cuda(), **kw)
    torch.cuda.synchronize()
    return q, x, book, vq_book, codes.cpu().numpy(), None if labels is None else labels.cpu().numpy().astype(np.int64)


def counters():
    from cuvs_amd._lib import lib

    """(default encoder launches, plain encoder launches, default launches with more than one row per lane)"""
    out = (C.c_ulonglong * 3)()
    lib().cuvsAmdPqEncodeCounters(out)
    return int(out[0]), int(out[1]), int(out[2])


def num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def all_cases():
    return P.ENCODER_CASES + P.PARITY_ONLY_CASES + P.multi_row_cases(num_cus())


def main(path):
    out = {}
    for i, case in enumerate(all_cases()):
        _, _, _, _, codes, labels = encode_case(case)
        out[f"codes{i}"] = codes
        if labels is not None:
            out[f"labels{i}"] = labels
    out["counters"] = np.array(counters())
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])

"""numpy side of the CAGRA VPQ tests: the decode of a compressed dataset, and a parser / writer of the reference's CAGRA file
whose dataset record is a VPQ dataset (tag 3), restated from the serializer (detail/dataset_serialize.hpp:59-73,102-111;
scalar types from the vpq_dataset<half, int64_t> accessors: n_rows int64, the other five uint32).

A row of `codes` is [uint32 VQ label][pq_dim code bytes][zero padding to a multiple of 4 bytes]."""
import numpy as np

from tests import refformat as rf

TAG_VPQ = 3
CUDA_R_16F, CUDA_R_32F = 2, 0


def row_len(pq_dim):
    """bytes of an encoded row: 4 * (1 + ceil(pq_dim * 8 / 32))"""
    return 4 * (1 + -(-pq_dim // 4))


def split_codes(codes, pq_dim):
    """codes uint8 [n, row_len] -> (labels uint32 [n], pq codes uint8 [n, pq_dim], padding bytes uint8 [n, *])"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    assert codes.shape[1] == row_len(pq_dim)
    labels = codes[:, :4].copy().view("<u4")[:, 0]
    return labels, codes[:, 4:4 + pq_dim], codes[:, 4 + pq_dim:]


def join_codes(labels, pq_codes):
    n, pq_dim = pq_codes.shape
    out = np.zeros((n, row_len(pq_dim)), np.uint8)
    out[:, :4] = np.asarray(labels, "<u4").reshape(n, 1).view(np.uint8)
    out[:, 4:4 + pq_dim] = pq_codes
    return out


def decode(vq_book, pq_book, codes):
    """x[i, d] = float32(vq_book[label_i, d]) + float32(pq_book[code_i[d // pq_len], d % pq_len]): one fp32 addition"""
    vq = np.asarray(vq_book).astype(np.float32)
    pq = np.asarray(pq_book).astype(np.float32)
    dim, pq_len = vq.shape[1], pq.shape[1]
    labels, c, _ = split_codes(codes, dim // pq_len)
    return (vq[labels] + pq[c].reshape(len(c), dim)).astype(np.float32)


def parse_cagra_vpq(path):
    """the whole file; the dataset record must be a VPQ dataset"""
    with open(path, "rb") as f:
        out = {"prefix": f.read(4), "version": rf.scalar(f)}
        out["size"], out["dim"], out["graph_degree"], out["metric"] = rf.scalar(f), rf.scalar(f), rf.scalar(f), rf.scalar(f)
        out["graph"] = rf.read_record(f)
        out["content_map"] = rf.scalar(f)
        assert out["content_map"] & 1
        for key, dt in (("tag", np.uint32), ("cuda_dtype", np.uint32), ("n_rows", np.int64), ("ds_dim", np.uint32),
                        ("vq_n_centers", np.uint32), ("pq_n_centers", np.uint32), ("pq_len", np.uint32),
                        ("encoded_row_length", np.uint32)):
            a = rf.read_record(f)
            assert a.shape == () and a.dtype == np.dtype(dt), (key, a.dtype)
            out[key] = a.item()
        assert out["tag"] == TAG_VPQ
        out["vq_code_book"], out["pq_code_book"], out["data"] = rf.read_record(f), rf.read_record(f), rf.read_record(f)
        if out["content_map"] & 2:
            out["source_indices"] = rf.read_record(f)
        assert f.read(1) == b""
    return out


def write_cagra_vpq(path, graph, vq_book, pq_book, codes, dtype=np.float32, metric=0, book_dtype=np.float16, **override):
    """override: header scalars written instead of the true ones (pq_n_centers, pq_len, encoded_row_length)"""
    dtype = np.dtype(dtype)
    head = {"n_rows": codes.shape[0], "ds_dim": vq_book.shape[1], "vq_n_centers": vq_book.shape[0], "pq_n_centers": pq_book.shape[0],
            "pq_len": pq_book.shape[1], "encoded_row_length": codes.shape[1]}
    head.update(override)
    with open(path, "wb") as f:
        f.write(rf.PREFIX[dtype])
        rf.write_scalar(f, 5, np.int32)
        rf.write_scalar(f, graph.shape[0], np.uint32)
        rf.write_scalar(f, vq_book.shape[1], np.uint32)
        rf.write_scalar(f, graph.shape[1], np.uint32)
        rf.write_scalar(f, metric, np.int32)
        rf.write_record(f, graph.astype(np.uint32))
        rf.write_scalar(f, 1, np.uint32)
        rf.write_scalar(f, TAG_VPQ, np.uint32)
        rf.write_scalar(f, CUDA_R_16F if np.dtype(book_dtype) == np.float16 else CUDA_R_32F, np.uint32)
        rf.write_scalar(f, head["n_rows"], np.int64)
        for key in ("ds_dim", "vq_n_centers", "pq_n_centers", "pq_len", "encoded_row_length"):
            rf.write_scalar(f, head[key], np.uint32)
        rf.write_record(f, np.asarray(vq_book).astype(book_dtype))
        rf.write_record(f, np.asarray(pq_book).astype(book_dtype))
        rf.write_record(f, np.ascontiguousarray(codes, dtype=np.uint8))

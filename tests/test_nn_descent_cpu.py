"""CPU: the NN-descent twin (tests/nn_descent_ref.py) against brute-force definitions on tiny inputs. The GPU tests compare
the kernels with the twin; this file is what the twin itself answers to."""
import numpy as np
import pytest

from tests import nn_descent_ref as R

NEW, NONE = R.NEW, R.NONE


def _rows(rng, n, dim, dtype):
    if dtype == np.int8:
        return rng.integers(-128, 128, (n, dim)).astype(np.int8)
    if dtype == np.uint8:
        return rng.integers(0, 256, (n, dim)).astype(np.uint8)
    return (rng.standard_normal((n, dim)) * 2.0 + 0.1).astype(dtype)


def test_keys_keep_the_order_of_floats_and_round_trip():
    f = np.array([-np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-30, 2.0, 3.4e38, np.inf], np.float32)
    k = R.float_to_key(f)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert (R.key_to_float(k).view(np.uint32) == f.view(np.uint32)).all()
    assert R.float_to_key(np.float32(np.nan)) > k[-1]          # the NaN a 0/0 cosine would make sorts behind +inf


@pytest.mark.parametrize("dtype", [np.float32, np.float16, np.int8, np.uint8])
@pytest.mark.parametrize("metric", ["sqeuclidean", "inner_product", "cosine"])
@pytest.mark.parametrize("dim", [1, 7, 8, 31, 64, 100, 136, 515])
def test_pair_key_against_float64(dtype, metric, dim):
    rng = np.random.default_rng(dim)
    n = 40
    x = _rows(rng, n, dim, dtype)
    a, b = rng.integers(0, n, 300), rng.integers(0, n, 300)
    norms = R.row_norms(x)
    got = R.key_to_float(R.pair_keys(x, a, b, metric, norms)).astype(np.float64)
    if metric == "inner_product":
        got = -got
    want, bound = R.exact_distance_and_bound(x, a, b, metric, norm_rel_err=R.U + 2.0 ** -40)   # R.row_norms: one fp32 rounding
    err = np.abs(got - want)
    assert (err <= bound).all(), (err.max(), bound[err.argmax()])
    if metric == "sqeuclidean":
        assert (got[a == b] == 0).all()


@pytest.mark.parametrize("dtype", [np.int8, np.uint8])
@pytest.mark.parametrize("dim", [1, 15, 16, 24, 33, 129, 256])
def test_pair_key_of_integer_rows_is_exact(dtype, dim):
    """|x| <= 255 and dim <= 256: every partial sum is an integer below 2^24 - exact in fp32 in any order."""
    rng = np.random.default_rng(100 + dim)
    n = 30
    x = _rows(rng, n, dim, dtype)
    a, b = rng.integers(0, n, 200), rng.integers(0, n, 200)
    xi = x.astype(np.int64)
    l2 = ((xi[a] - xi[b]) ** 2).sum(1)
    ip = (xi[a] * xi[b]).sum(1)
    assert l2.max() < 2 ** 24 and np.abs(ip).max() < 2 ** 24
    assert (R.key_to_float(R.pair_keys(x, a, b, "sqeuclidean")) == l2).all()
    assert (-R.key_to_float(R.pair_keys(x, a, b, "inner_product")) == ip).all()
    ham = np.array([sum(bin(int(p) ^ int(q)).count("1") for p, q in zip(x.view(np.uint8)[i], x.view(np.uint8)[j]))
                    for i, j in zip(a, b)])
    assert (R.key_to_float(R.pair_keys(x, a, b, "bitwise_hamming")) == ham).all()


def test_cosine_key_of_a_zero_row_is_zero():
    x = np.array([[0, 0, 0], [1, 2, 3], [-1, 0, 2]], np.float32)
    k = R.pair_keys(x, [0, 1, 0, 1], [1, 0, 0, 2], "cosine", R.row_norms(x))
    d = R.key_to_float(k)
    nr = R.row_norms(x)
    assert np.isfinite(d).all() and (d[:3] == 0).all() and d[3] == np.float32(1) - np.float32(5) / (nr[1] * nr[2])


def _merge_by_definition(v, ids, keys, pids, pkeys, cnt, K):
    """python sorted + dict: the best copy of every id, a listed copy before a proposed one"""
    ent = [(int(k), int(i) & 0x7FFFFFFF, int(i) >> 31) for i, k in zip(ids, keys) if i != NONE]
    ent += [(int(k), int(i), 1) for i, k in zip(pids[:cnt], pkeys[:cnt]) if i != NONE and i != v]
    best = {}
    for k, i, f in sorted(ent):
        best.setdefault(i, (k, i, f))          # the first in (key, id, flag) order: the list's copy on equal keys
    kept = sorted(best.values())[:K]
    oi = [i | (f << 31) for _, i, f in kept] + [NONE] * (K - len(kept))
    ok = [k for k, _, _ in kept] + [NONE] * (K - len(kept))
    return oi, ok, (ok[K - 1] if len(kept) == K else NONE)


@pytest.mark.parametrize("K,P,n_ids", [(4, 64, 12), (5, 64, 40), (32, 64, 50), (33, 66, 200)])
def test_merge_twin_against_sorted_and_dict(K, P, n_ids):
    rng = np.random.default_rng(K)
    n = 9
    key_of = lambda v, u: np.uint32(0x80000000 + ((v * 7919 + u * 104729) % 23))       # few distinct keys: many ties
    ids = np.full((n, K), NONE, np.uint32); keys = np.full((n, K), NONE, np.uint32)
    pids = rng.integers(0, n_ids, (n, P)).astype(np.uint32)
    pids[rng.random((n, P)) < 0.05] = NONE
    cnt = rng.integers(0, P + 8, n).astype(np.uint32)
    cnt[0], cnt[1] = 0, P + 7
    for v in range(n):
        m = int(rng.integers(0, K + 1))
        cand = rng.permutation([u for u in range(n_ids) if u != v])[:m]
        ent = sorted((int(key_of(v, u)), int(u)) for u in cand)
        for s, (k, u) in enumerate(ent):
            ids[v, s] = u | (NEW if rng.random() < 0.5 else 0)
            keys[v, s] = k
    pkeys = np.array([[key_of(v, u) if u != NONE else 12345 for u in pids[v]] for v in range(n)], np.uint32)
    oi, ok, worst, pc = R.merge(ids, keys, pids, pkeys, cnt)
    assert (pc == 0).all()
    for v in range(n):
        wi, wk, ww = _merge_by_definition(v, ids[v], keys[v], pids[v], pkeys[v], min(int(cnt[v]), P), K)
        assert oi[v].tolist() == wi and ok[v].tolist() == wk and int(worst[v]) == ww


def test_sample_twin_on_a_hand_made_list():
    ids = np.full((40, 40), NONE, np.uint32)
    ids[0, :36] = np.arange(1, 37)            # 36 old entries: the first 32 are sampled
    ids[0, 36:38] = [2 | NEW, 1 | NEW]
    ids[1, :3] = [0 | NEW, 2, 3 | NEW]
    s = R.sample(ids)
    assert s["fwd_new"][0, :3].tolist() == [2, 1, NONE] and s["fwd_old"][0].tolist() == list(range(1, 33))
    assert s["fwd_new"][1, :3].tolist() == [0, 3, NONE] and s["fwd_old"][1, :2].tolist() == [2, NONE]
    assert ((s["ids"] & np.uint32(NEW))[s["ids"] != NONE] == 0).all() and (s["ids"][0, 36:38] == [2, 1]).all()
    assert s["rev_new_cnt"][:5].tolist() == [1, 1, 1, 1, 0] and s["rev_new_set"][2] == [0] and s["rev_new_set"][0] == [1]
    assert s["rev_old_cnt"].sum() == 32 + 1 and s["rev_old_set"][2] == [0, 1] and s["rev_old_cnt"][33] == 0


def test_join_twin_counts_pairs_on_a_hand_made_case():
    x = np.arange(12, dtype=np.float32).reshape(6, 2)
    none = np.full((6, R.S), NONE, np.uint32)
    fn, fo, rn, ro = none.copy(), none.copy(), none.copy(), none.copy()
    fn[0, :3] = [1, 2, 3]                     # 3 new-new pairs
    fo[0, :2] = [4, 2]                        # 3 x 2 new-old pairs, one of them (2, 2): skipped
    rn[0, :2] = [5, 9999]                     # the count says 1: the second slot is not read
    cnt, props = R.join(x, "sqeuclidean", None, fn, fo, rn, ro, np.array([1, 0, 0, 0, 0, 0]), np.zeros(6), np.full(6, NONE))
    # cn = {1, 2, 3, 5}: 6 pairs; cn x co = 8 pairs, minus (2, 2): 13 pairs, two proposals each
    assert cnt.sum() == 26 and cnt[0] == 0
    assert props[4] == sorted((u, int(R.float_to_key(np.float32(((x[4] - x[u]) ** 2).sum())))) for u in (1, 2, 3, 5))
    worst = np.full(6, NONE, np.uint32)
    worst[4] = R.float_to_key(np.float32(32.0))           # row 4 only takes keys below 32: rows 3 and 5 (8) - not row 2 (32)
    cnt2, props2 = R.join(x, "sqeuclidean", None, fn, fo, rn, ro, np.array([1, 0, 0, 0, 0, 0]), np.zeros(6), worst)
    assert [u for u, _ in props2[4]] == [3, 5] and cnt2[4] == 2


def test_init_twin_slot_rules():
    rng = np.random.default_rng(5)
    n, K, P, seed = 23, 8, 64, 0x9E3779B97F4A7C15
    x = rng.standard_normal((n, 5)).astype(np.float32)
    u, keys, cnt = R.init(x, "sqeuclidean", None, K, P, seed)
    assert u.shape == (n, K) and (cnt == K).all() and (u < n).all() and (u != np.arange(n)[:, None]).all()
    assert (keys == R.pair_keys(x, np.repeat(np.arange(n), K), u.ravel(), "sqeuclidean").reshape(n, K)).all()
    v, c = 3, 5
    z = (v * K + c) ^ seed
    z ^= z >> 12; z = (z ^ (z << 25)) & (2 ** 64 - 1); z ^= z >> 27
    r = (z * 0x2545F4914F6CDD1D & (2 ** 64 - 1)) % n
    assert u[v, c] == (r if r != v else (r + 1) % n)
    # clusters {5, 1, 7}, {0}, {2, 3}, the rest; hubs 9 and 1
    perm = np.array([5, 1, 7, 0, 2, 3] + [i for i in range(n) if i not in (5, 1, 7, 0, 2, 3)], np.uint32)
    cl_off = np.array([0, 3, 4, 6, n], np.uint32)
    labels = np.empty(n, np.uint32)
    for L in range(4):
        labels[perm[cl_off[L]:cl_off[L + 1]]] = L
    uc, _, _ = R.init(x, "sqeuclidean", None, K, P, seed, perm, cl_off, labels, hubs=[9, 1])
    assert uc[1, 0] == 7 and uc[1, 2] == 5 and uc[1, 4] == u[1, 4]       # two mates, then random again
    assert uc[0, 0] == u[0, 0] and uc[2, 0] == 3 and uc[2, 2] == u[2, 2]   # clusters of one and two rows
    assert (uc[:, 3] == np.where(np.arange(n) == 9, 10, 9)).all() and uc[5, 7] == 1 and uc[1, 7] == 2
    assert (uc[:, 1::2][:, ::2] == u[:, 1::2][:, ::2]).all()                # slots 1 and 5 stay random

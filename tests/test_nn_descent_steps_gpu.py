"""GPU: every NN-descent kernel, launched alone through the cuvsAmdNnDescentStep hook (the launches nnd_run makes), against the
CPU twin tests/nn_descent_ref.py - equality, not recall. What depends on atomic order (which 32 of more publishers a reverse
list keeps, which P of more proposals a buffer keeps, the order inside either) is compared as a set / multiset."""
import collections
import ctypes as C

import numpy as np
import pytest

from tests import nn_descent_ref as R

pytestmark = pytest.mark.gpu

NEW, NONE, S = R.NEW, R.NONE, R.S
INIT, MERGE, SAMPLE, JOIN, COUNT_NEW = range(5)
ELEM = {np.dtype(np.float32): 0, np.dtype(np.float16): 1, np.dtype(np.int8): 2, np.dtype(np.uint8): 3}
POISON = 0xDEADBEEF


class _Args(C.Structure):
    _fields_ = ([(name, C.c_void_p) for name in ("ids", "keys", "worst", "prop_ids", "prop_keys", "prop_cnt", "fwd_new", "fwd_old",
                                                  "rev_new", "rev_old", "rev_new_cnt", "rev_old_cnt", "n_updates")]
                + [("n", C.c_int64), ("K", C.c_uint32), ("P", C.c_uint32), ("data", C.c_void_p), ("dim", C.c_int64),
                   ("elem", C.c_int32), ("metric", C.c_int32), ("norms", C.c_void_p), ("seed", C.c_uint64), ("perm", C.c_void_p),
                   ("pos_of", C.c_void_p), ("cl_off", C.c_void_p), ("labels", C.c_void_p), ("hubs", C.c_void_p),
                   ("n_hubs", C.c_uint32)])


def _dev(a):
    """numpy array -> device tensor with the same bits (torch has no uint32: int32 carries them)"""
    import torch

    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).cuda()


def _host(t, dtype=np.uint32):
    return t.cpu().numpy().view(dtype)


class _State:
    """The device arrays of one nnd_state: given ones uploaded, the others poisoned."""
    SHAPES = dict(ids="K", keys="K", worst=None, prop_ids="P", prop_keys="P", prop_cnt=None, fwd_new=S, fwd_old=S, rev_new=S,
                  rev_old=S, rev_new_cnt=None, rev_old_cnt=None)

    def __init__(self, n, K, P, **given):
        self.n, self.K, self.P = n, K, P
        self.t = {}
        for name, cols in self.SHAPES.items():
            cols = {"K": K, "P": P}.get(cols, cols)
            shape = (n,) if cols is None else (n, cols)
            a = given.pop(name, None)
            a = np.full(shape, POISON, np.uint32) if a is None else np.asarray(a, np.uint32)
            assert a.shape == shape, (name, a.shape, shape)
            self.t[name] = _dev(a)
        self.t["n_updates"] = _dev(np.zeros(1, np.uint64))
        assert not given, given

    def get(self, name):
        return _host(self.t[name], np.uint64 if name == "n_updates" else np.uint32)

    def step(self, res, step, x=None, metric="sqeuclidean", norms=None, seed=0, perm=None, cl_off=None, labels=None, hubs=None):
        from cuvs_amd._lib import check, lib
        from cuvs_amd.distance import DISTANCE_TYPES

        a = _Args()
        for name, t in self.t.items():
            setattr(a, name, t.data_ptr())
        a.n, a.K, a.P, a.seed, a.metric = self.n, self.K, self.P, seed, DISTANCE_TYPES[metric]
        keep = []
        if x is not None:   # a device tensor (the caller chooses its base address)
            a.data, a.dim, a.elem = x.data_ptr(), x.shape[1], ELEM[np.dtype(str(x.dtype).replace("torch.", ""))]
        if norms is not None:
            keep.append(_dev(np.asarray(norms, np.float32)))
            a.norms = keep[-1].data_ptr()
        if perm is not None:
            pos_of = np.empty(self.n, np.uint32)
            pos_of[np.asarray(perm)] = np.arange(self.n)
            for name, arr in (("perm", perm), ("pos_of", pos_of), ("cl_off", cl_off), ("labels", labels)):
                keep.append(_dev(np.asarray(arr, np.uint32)))
                setattr(a, name, keep[-1].data_ptr())
        if hubs is not None:
            keep.append(_dev(np.asarray(hubs, np.uint32)))
            a.hubs, a.n_hubs = keep[-1].data_ptr(), len(hubs)
        fn = lib().cuvsAmdNnDescentStep
        fn.restype = C.c_int
        check(fn(res.get_c_obj(), C.c_int(step), C.byref(a)))
        res.sync()


# --------------------------------------------------------------------------------------------------------------- merge
SCENARIOS = ("random", "all_listed", "five_times", "one_key", "self_and_none", "short")


def _pair_key(v, u, n_keys):
    """the same pair has the same key (the invariant the kernel states); few values, so that different ids tie"""
    return 0x80000000 + (v * 2654435761 + u * 40503) % 1000003 % n_keys


def _merge_row(rng, v, K, P, cnt, scenario):
    """one row's list and proposal buffer -> (ids [K], keys [K], prop_ids [P], prop_keys [P])"""
    universe = [u for u in range(4 * K + 16) if u != v]
    n_keys = 1 if scenario == "one_key" else 3 * K
    fill = {"all_listed": K, "short": 0}.get(scenario, int(rng.integers(0, K + 1)))
    listed = rng.permutation(universe)[:fill].tolist()
    ent = sorted((_pair_key(v, u, n_keys), u) for u in listed)
    ids, keys = np.full(K, NONE, np.uint32), np.full(K, NONE, np.uint32)
    for s, (k, u) in enumerate(ent):
        ids[s], keys[s] = u | (NEW if rng.random() < 0.5 else 0), k
    live = min(cnt, P)
    if scenario == "all_listed":
        prop = rng.choice(listed, live).tolist()
    elif scenario == "short":
        prop = rng.choice(universe[:max(1, K // 2)], live).tolist()          # fewer than K distinct ids in all
    else:
        prop = rng.choice(universe, live).tolist()
    if scenario == "five_times" and live >= 5:
        fresh = next(u for u in universe if u not in listed)
        for s in rng.permutation(live)[:5]:
            prop[s] = fresh
    if scenario == "self_and_none":
        for s in range(live):
            prop[s] = (v, NONE, prop[s])[int(rng.integers(0, 3))]
    pids, pkeys = np.empty(P, np.uint32), np.empty(P, np.uint32)
    for s in range(P):
        if s < live:
            pids[s] = prop[s]
            pkeys[s] = _pair_key(v, prop[s], n_keys) if prop[s] != NONE else POISON
        else:   # past the count: an id nobody lists with the best key there is - it must not be read
            pids[s], pkeys[s] = 0x70000000 + s, 0
    return ids, keys, pids, pkeys


@pytest.mark.parametrize("n", [1, 3, 5, 9])
@pytest.mark.parametrize("K", [4, 32, 33, 64, 96, 160])
def test_merge(K, n, res):
    P = max(64, 2 * K)
    combos = [(sc, c) for sc in SCENARIOS for c in (0, 1, P, P + 7)]
    rng = np.random.default_rng(1000 * K + n)
    seen_short = False
    for start in range(0, len(combos), n):
        rows = [combos[(start + v) % len(combos)] for v in range(n)]
        parts = [_merge_row(rng, v, K, P, cnt, sc) for v, (sc, cnt) in enumerate(rows)]
        ids, keys, pids, pkeys = (np.stack([p[i] for p in parts]) for i in range(4))
        cnt = np.array([c for _, c in rows], np.uint32)
        st = _State(n, K, P, ids=ids, keys=keys, prop_ids=pids, prop_keys=pkeys, prop_cnt=cnt)
        st.step(res, MERGE)
        wi, wk, ww, wc = R.merge(ids, keys, pids, pkeys, cnt)
        label = f"K {K} rows {rows}"
        np.testing.assert_array_equal(st.get("ids"), wi, label)
        np.testing.assert_array_equal(st.get("keys"), wk, label)
        np.testing.assert_array_equal(st.get("worst"), ww, label)
        np.testing.assert_array_equal(st.get("prop_cnt"), wc, label)
        seen_short |= bool(((wi[:, -1] == NONE) & (ww == NONE)).any())
        for v, (sc, c) in enumerate(rows):   # the properties the twin stands for, stated directly
            if sc == "all_listed":           # nothing new: the list and its flags survive
                assert (wi[v] == ids[v]).all() and (wk[v] == keys[v]).all()
            bare = wi[v][wi[v] != NONE] & 0x7FFFFFFF
            assert len(set(bare.tolist())) == bare.size and v not in bare and (bare < 0x70000000).all()
    assert seen_short


# -------------------------------------------------------------------------------------------------------------- sample
@pytest.mark.parametrize("K", [8, 64, 96])
def test_sample(K, res):
    rng = np.random.default_rng(K)
    n, hub = 121, 7                                                        # 4 rows per workgroup: the last one has idle waves
    ids = np.full((n, K), NONE, np.uint32)
    for v in range(n):
        fill = K if v % 3 else int(rng.integers(0, K + 1))               # every third row has a 0xffffffff tail
        others = [u for u in range(n) if u not in (v, hub)]
        row = rng.permutation(others)[:fill].astype(np.uint32)
        row |= np.where(rng.random(fill) < 0.5, np.uint32(NEW), np.uint32(0))
        if fill and v != hub:
            row[0] = hub | NEW                                             # the hub: listed as new by (nearly) every row
        ids[v, :fill] = row
    if K == 96:   # 50 flagged entries in one list: 32 are sampled, 18 keep their flag
        row = rng.permutation([u for u in range(n) if u != 1])[:K].astype(np.uint32)
        row[rng.permutation(K)[:50]] |= np.uint32(NEW)
        ids[1] = row
    st = _State(n, K, 64, ids=ids, rev_new_cnt=np.zeros(n), rev_old_cnt=np.zeros(n))
    st.step(res, SAMPLE)
    want = R.sample(ids)
    for name in ("ids", "fwd_new", "fwd_old", "rev_new_cnt", "rev_old_cnt"):
        np.testing.assert_array_equal(st.get(name), want[name], name)
    assert want["rev_new_cnt"][hub] > S
    if K == 96:
        got = st.get("ids")[1]
        assert int(((got & NEW) != 0).sum()) == 18 and (got & 0x7FFFFFFF == ids[1] & 0x7FFFFFFF).all()
    for kind in ("new", "old"):
        rev, cnt = st.get(f"rev_{kind}"), want[f"rev_{kind}_cnt"]
        for u in range(n):
            expect = want[f"rev_{kind}_set"][u]
            got = rev[u, :min(int(cnt[u]), S)].tolist()
            if cnt[u] <= S:
                assert sorted(got) == expect, (kind, u)
            else:
                assert len(set(got)) == S and set(got) <= set(expect), (kind, u)
            assert (rev[u, min(int(cnt[u]), S):] == POISON).all()     # nothing written past the count


def test_count_new(res):
    rng = np.random.default_rng(9)
    n, K = 37, 33                                                      # n K = 1221: the last workgroup is part full
    ids = rng.integers(0, n, (n, K)).astype(np.uint32) | np.where(rng.random((n, K)) < 0.3, np.uint32(NEW), np.uint32(0))
    ids[rng.random((n, K)) < 0.2] = NONE                               # an empty slot has the flag's bit set and does not count
    st = _State(n, K, 64, ids=ids)
    st.step(res, COUNT_NEW)
    assert int(st.get("n_updates")[0]) == R.count_new(ids) > 0


# ---------------------------------------------------------------------------------------------------------------- join
def _rows(rng, n, dim, dtype, metric):
    if metric == "bitwise_hamming":
        return rng.integers(0, 256, (n, dim)).astype(np.uint8).view(dtype)
    if dtype == np.int8:
        return rng.integers(-5, 5, (n, dim)).astype(np.int8)
    if dtype == np.uint8:
        return rng.integers(0, 5, (n, dim)).astype(np.uint8)
    return (rng.standard_normal((n, dim)) * 2.0 + 0.1).astype(dtype)


def _join_case(x, metric, res, x_dev=None):
    """Rows 0-7: Nn in {0, 1, 2, 64} x No in {0, 64} (64 = 32 forward + 32 of MORE reverse entries); row 8: ids shared between
    the forward and the reverse samples and between new and old; row 5 of the data is a zero row and is sampled."""
    n, K, P = x.shape[0], 32, 64
    rng = np.random.default_rng(x.shape[1])
    zero = 5
    fwd = {k: np.full((n, S), NONE, np.uint32) for k in ("new", "old")}
    rev = {k: np.full((n, S), POISON, np.uint32) for k in ("new", "old")}
    cnt = {k: np.zeros(n, np.uint32) for k in ("new", "old")}

    def fill(v, kind, total):
        ids = rng.permutation(n)[:total].astype(np.uint32)
        if total >= 2:
            ids[1] = zero
        f = min(total, S) if total != 1 else 1
        fwd[kind][v, :f] = ids[:f]
        if total > f:
            rev[kind][v, :total - f] = ids[f:]
            cnt[kind][v] = total - f + 13          # more publishers than slots: the 32 slots are read, not 45
        elif v % 2:
            rev[kind][v, :3] = rng.integers(0, n, 3)   # a count of 0 over stale slots: they are not read
    for v, (nn, no) in enumerate((a, b) for a in (0, 1, 2, 64) for b in (0, 64)):
        fill(v, "new", nn)
        fill(v, "old", no)
    fwd["new"][8, :3], rev["new"][8, :2], cnt["new"][8] = [20, 21, 22], [20, 23], 2
    fwd["old"][8, :2], rev["old"][8, :1], cnt["old"][8] = [21, 24], [24], 1
    keys_all = R.pair_keys(x, rng.integers(0, n, 4000), rng.integers(0, n, 4000), metric, R.row_norms(x))
    worst = np.where(rng.random(n) < 0.5, np.uint32(NONE), np.uint32(np.median(keys_all)))   # every second row is selective
    norms = R.row_norms(x) if metric == "cosine" else None
    st = _State(n, K, P, worst=worst, prop_cnt=np.zeros(n), fwd_new=fwd["new"], fwd_old=fwd["old"], rev_new=rev["new"],
                rev_old=rev["old"], rev_new_cnt=cnt["new"], rev_old_cnt=cnt["old"])
    st.step(res, JOIN, x=_dev(x) if x_dev is None else x_dev, metric=metric, norms=norms)
    want_cnt, want = R.join(x, metric, norms, fwd["new"], fwd["old"], rev["new"], rev["old"], cnt["new"], cnt["old"], worst)
    np.testing.assert_array_equal(st.get("prop_cnt"), want_cnt)
    pi, pk = st.get("prop_ids"), st.get("prop_keys")
    for t in range(n):
        c = int(want_cnt[t])
        got = sorted(zip(pi[t, :min(c, P)].tolist(), pk[t, :min(c, P)].tolist()))
        if c <= P:
            assert got == want[t], t
        else:
            assert not collections.Counter(got) - collections.Counter(want[t]), t
        assert (pi[t, min(c, P):] == POISON).all()
    assert (want_cnt > P).any() and ((want_cnt > 0) & (want_cnt <= P)).any()   # both ends of the overflow rule were met
    if metric == "cosine":
        zk = [k for t in range(n) for u, k in want[t] if zero in (t, u)]
        assert zk and all(k == R.float_to_key(np.float32(0.0)) for k in zk)


@pytest.mark.parametrize("dim", [1, 7, 8, 31, 64, 100, 136])
@pytest.mark.parametrize("metric", ["sqeuclidean", "inner_product", "cosine"])
@pytest.mark.parametrize("dtype", [np.float32, np.float16, np.int8, np.uint8], ids=["f32", "f16", "i8", "u8"])
def test_join(dtype, metric, dim, res):
    x = _rows(np.random.default_rng(dim), 150, dim, dtype, metric)
    x[5] = 0
    _join_case(x, metric, res)


@pytest.mark.parametrize("dim", [16, 24, 33, 136, 160])     # 16, 160: whole 16-byte pieces; 136, 160: more than one team pass
@pytest.mark.parametrize("dtype", [np.int8, np.uint8], ids=["i8", "u8"])
def test_join_hamming(dtype, dim, res):
    x = _rows(np.random.default_rng(dim), 150, dim, dtype, "bitwise_hamming")
    x[5] = 0
    _join_case(x, "bitwise_hamming", res)


@pytest.mark.parametrize("dim,skip", [(24, 24), (16, 8)])
def test_join_hamming_rows_off_16_byte_alignment(dim, skip, res):
    """dim 24: a row sliced off a [n + 1, 24] tensor; dim 16: whole pieces behind a base 8 bytes off - both take the byte branch"""
    x = _rows(np.random.default_rng(dim), 150, dim, np.uint8, "bitwise_hamming")
    x[5] = 0
    flat = _dev(np.concatenate([np.full(skip, 0xFF, np.uint8), x.ravel()]))
    x_dev = flat[skip:].view(150, dim)
    assert x_dev.data_ptr() % 16 == 8
    _join_case(x, "bitwise_hamming", res, x_dev=x_dev)


# ---------------------------------------------------------------------------------------------------------------- init
def _clusters(n):
    """rows grouped by hand: clusters of 1, 2, 3 and 9 rows, the rest in one"""
    perm = np.random.default_rng(n).permutation(n).astype(np.uint32)
    cl_off = np.array([0, 1, 3, 6, 15, n], np.uint32)
    labels = np.empty(n, np.uint32)
    for L in range(len(cl_off) - 1):
        labels[perm[cl_off[L]:cl_off[L + 1]]] = L
    return perm, cl_off, labels


@pytest.mark.parametrize("setup", ["plain", "clusters", "clusters+hubs", "hubs"])
@pytest.mark.parametrize("dtype,metric,dim,K", [(np.float32, "sqeuclidean", 100, 8), (np.float16, "cosine", 31, 40),
                                                (np.int8, "inner_product", 136, 33), (np.uint8, "bitwise_hamming", 24, 70)],
                         ids=["f32-l2", "f16-cos", "i8-ip", "u8-ham"])
def test_init(dtype, metric, dim, K, setup, res):
    n, P, seed = 61, max(64, 2 * K), 0x9E3779B97F4A7C15
    x = _rows(np.random.default_rng(K), n, dim, dtype, metric)
    x[11] = 0
    norms = R.row_norms(x) if metric == "cosine" else None
    kw = {}
    if "clusters" in setup:
        kw["perm"], kw["cl_off"], kw["labels"] = _clusters(n)
    if "hubs" in setup:
        kw["hubs"] = [17, 3, 11][:max(1, min(3, K // 4 - 1))]    # fewer hubs than fourth slots: the other ones stay random
        assert len(kw["hubs"]) < K // 4
    st = _State(n, K, P)
    st.step(res, INIT, x=_dev(x), metric=metric, norms=norms, seed=seed, **kw)
    wi, wk, wc = R.init(x, metric, norms, K, P, seed, **kw)
    c = min(K, P)
    np.testing.assert_array_equal(st.get("prop_ids")[:, :c], wi)
    np.testing.assert_array_equal(st.get("prop_keys")[:, :c], wk)
    np.testing.assert_array_equal(st.get("prop_cnt"), wc)
    assert (st.get("prop_ids")[:, c:] == POISON).all()
    plain = R.init(x, metric, norms, K, P, seed)[0]
    assert (setup == "plain") == bool((wi == plain).all())          # the clustering and the hubs did change slots

"""GPU: cuvs_amd.distance.masked_l2_nn and cross_component_nn (cuvs_amd/csrc/masked_nn.hip) against the fp64 numpy reference
tests/masked_nn_ref.py. Integer rows in [-3, 3] make every product, sum and norm exact in fp32, so ids and
distances are compared bit for bit, ties included; Gaussian rows are held to the rounding bound derived in DESIGN."""
import numpy as np
import pytest
import torch

from tests import masked_nn_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (130, 257, 20, 3), (200, 300, 16, 70), (129, 128, 33, 5)]
ids = lambda c: "x".join(map(str, c))  # noqa: E731


def D():
    from cuvs_amd import distance

    return distance


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(res, x, y, adj, ends, sqrt=False, out=None):
    idx, dist = D().masked_l2_nn(dev(x), dev(y), dev(adj), dev(ends), sqrt=sqrt, out=out, resources=res)
    res.sync()
    return idx.cpu().numpy(), dist.cpu().numpy()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


@pytest.mark.parametrize("sqrt", [False, True], ids=["sq", "sqrt"])
@pytest.mark.parametrize("density", [0.5, 0.05])
@pytest.mark.parametrize("case", SHAPES, ids=ids)
def test_exact_on_integer_rows(res, case, density, sqrt):
    m, n, dim, G = case
    x, y, adj, ends = R.masked_case(m, n, dim, G, density)
    assert ends[-1] < n or n == 1
    want_idx, want_dist = R.masked_l2_nn(x, y, adj, ends, sqrt)
    idx, dist = run(res, x, y, adj, ends, sqrt)
    total, live = D().masked_nn_last_stats(res)
    print(case, density, sqrt, "tiles", total, "computed", live, "rows without a candidate", int((want_idx < 0).sum()))
    assert (idx == want_idx).all() and same_bits(dist, want_dist)
    assert m == 1 or (want_idx < 0).any()
    assert total == -(-m // 128) * -(-n // 128) and live <= total
    if n > 128:
        assert live < total  # rows 0..127 x columns 128..255 is switched off: the tile is not computed


def test_gaussian_rows_within_the_rounding_bound(res):
    m, n, dim, G = 200, 300, 20, 7
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal((m, dim)).astype(np.float32), rng.standard_normal((n, dim)).astype(np.float32)
    _, _, adj, ends = R.masked_case(m, n, dim, G, 0.5)
    idx, dist = run(res, x, y, adj, ends)
    d64 = R.sqdist64(x, y)
    want_idx, best = R.nearest(d64, R.admissible(adj, ends, n))
    assert ((idx < 0) == (want_idx < 0)).all()
    r = np.flatnonzero(idx >= 0)
    B = R.bound(x, y, d64)
    err = np.abs(dist[r].astype(np.float64) - d64[r, idx[r]])
    print("largest |dist - d64| / B =", (err / B[r, idx[r]]).max(), "picks that differ from fp64's:", int((idx != want_idx).sum()))
    assert (err <= B[r, idx[r]]).all()
    assert (d64[r, idx[r]] <= best[r] + B[r, idx[r]] + B[r, want_idx[r]]).all()
    assert R.admissible(adj, ends, n)[r, idx[r]].all()


@pytest.mark.parametrize("sqrt", [False, True], ids=["sq", "sqrt"])
def test_two_calls_over_complementary_masks_equal_one(res, sqrt):
    x, y, adj, ends = R.masked_case(200, 300, 16, 70, 0.5)
    half = np.random.default_rng(1).random(adj.shape) < 0.5
    one = run(res, x, y, adj, ends, sqrt)
    first = D().masked_l2_nn(dev(x), dev(y), dev(adj & half), dev(ends), sqrt=sqrt, resources=res)
    two = run(res, x, y, adj & ~half, ends, sqrt, out=first)
    assert (one[0] == two[0]).all() and same_bits(one[1], two[1])
    assert (one[0] == R.masked_l2_nn(x, y, adj, ends, sqrt)[0]).all()


def test_a_second_call_gives_the_same_bits(res):
    x, y, adj, ends = R.masked_case(200, 300, 20, 7, 0.5)
    rng = np.random.default_rng(2)
    x, y = rng.standard_normal(x.shape).astype(np.float32), rng.standard_normal(y.shape).astype(np.float32)
    a, b = run(res, x, y, adj, ends), run(res, x, y, adj, ends)
    assert (a[0] == b[0]).all() and same_bits(a[1], b[1])


@pytest.mark.parametrize("sqrt", [False, True], ids=["sq", "sqrt"])
@pytest.mark.parametrize("n_components", [1, 2, 37])
@pytest.mark.parametrize("n", [150, 400])
def test_cross_component(res, n, n_components, sqrt):
    rng = np.random.default_rng(n + n_components)
    x = R.int_rows(rng, n, 5)
    used = np.delete(np.arange(n_components), 3) if n_components > 3 else np.arange(n_components)  # colour 3 has no rows
    colors = rng.permutation(np.resize(used, n)).astype(np.int32)
    want = R.cross_component_nn(x, colors, n_components, sqrt)
    got = [t.cpu().numpy() for t in D().cross_component_nn(dev(x), dev(colors), n_components, sqrt=sqrt, resources=res)]
    for g, w in zip(got, want):
        assert same_bits(g, w) if w.dtype == np.float32 else (g == w).all()
    if n_components == 1:
        assert (got[0] == -1).all() and (got[1] == R.FLT_MAX).all() and got[2][0] == got[3][0] == -1 and got[4][0] == R.FLT_MAX
    else:
        assert (got[2][used] >= 0).all() and (colors[got[2][used]] == used).all() and (colors[got[3][used]] != used).all()


REFUSALS = {
    "dtype": (dict(ends=lambda e: e.to(torch.int32)), "group_idxs must be int64"),
    "host": (dict(x=lambda x: x.cpu()), "x must be accessible on device memory"),
    "adj_columns": (dict(adj=lambda a: a[:, :-1].contiguous()), "adj must have shape"),
    "widths": (dict(y=lambda y: y[:, :-1].contiguous()), "dim mismatch"),
    "colors_length": (dict(colors=lambda c: c[:-1].contiguous()), "colors must have shape"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_leave_the_outputs_alone(res, name):
    from cuvs_amd._lib import CuvsError

    change, message = REFUSALS[name]
    x, y, adj, ends = R.masked_case(130, 257, 20, 3, 0.5)
    a = dict(x=dev(x), y=dev(y), adj=dev(adj), ends=dev(ends), colors=dev(np.arange(130, dtype=np.int32) % 3))
    for key, f in change.items():
        a[key] = f(a[key])
    out = [torch.full((130,), 7, dtype=torch.int64).cuda(), torch.full((130,), 7.0).cuda(), torch.full((3,), 7, dtype=torch.int64).cuda(),
           torch.full((3,), 7, dtype=torch.int64).cuda(), torch.full((3,), 7.0).cuda()]
    with pytest.raises(CuvsError, match=message):
        if name == "colors_length":
            D().cross_component_nn(a["x"], a["colors"], 3, out=out, resources=res)
        else:
            D().masked_l2_nn(a["x"], a["y"], a["adj"], a["ends"], out=out[:2], resources=res)
    assert all((t == 7).all() for t in out)

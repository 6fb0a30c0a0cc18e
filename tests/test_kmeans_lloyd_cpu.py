"""CPU: the twin of the Lloyd fit's seeding (oracle.kmeans_seed_rows): its generator, Floyd's draw, that the k-means++
race samples proportionally to w * d^2 — and the trace of oracle.kmeans_lloyd. test_kmeans_lloyd_gpu.py holds the HIP
kernels to this twin pick for pick, which carries the sampling property over to them."""
import numpy as np
import pytest

import oracle


def test_mt19937_64_check_value():
    gen = oracle.mt19937_64(5489)  # [rand.predef]: the 10000th invocation of a default-constructed mt19937_64
    for _ in range(9999):
        gen()
    assert gen() == 9981545732273789042
    assert oracle.kmeans_trial_seeds(3) == oracle.kmeans_trial_seeds(5)[:3]
    gen0 = oracle.mt19937_64(0)
    assert oracle.kmeans_trial_seeds(2, seed=0) == [gen0(), gen0()]


@pytest.mark.parametrize("n,k", [(10, 10), (10, 1), (1, 1), (500, 7), (64, 63), (1000, 33), (5, 3)])
def test_floyd_draws_k_distinct_sorted_rows(n, k):
    x = np.zeros((n, 2), dtype=np.float32)
    seen = set()
    for seed in oracle.kmeans_trial_seeds(20):
        ids, trace = oracle.kmeans_seed_rows(x, k, "Random", seed)
        assert trace == [] and len(ids) == k and len(set(ids)) == k
        assert ids == sorted(ids) and 0 <= ids[0] and ids[-1] < n
        seen.add(tuple(ids))
    if k == n:
        assert seen == {tuple(range(n))}
    elif n >= 10:
        assert len(seen) > 1  # it does draw


def _chi2_quantile(dof, tail=1e-6):
    """The 1 - tail quantile of chi-square(dof)."""
    try:
        from scipy.stats import chi2
    except ImportError:  # Wilson-Hilferty: chi2_p ~ dof * (1 - 2/(9 dof) + z_p * sqrt(2/(9 dof)))^3
        z = 4.753424  # the 1 - 1e-6 quantile of the standard normal
        assert tail == 1e-6
        return dof * (1.0 - 2.0 / (9.0 * dof) + z * np.sqrt(2.0 / (9.0 * dof))) ** 3
    return float(chi2.ppf(1.0 - tail, dof))


@pytest.mark.parametrize("weighted", [False, True])
def test_the_race_draws_the_second_seed_proportionally_to_w_d2(weighted):
    n, trials = 32, 3000
    x = np.arange(n, dtype=np.float32)[:, None]  # 32 points on a line
    w = None
    if weighted:
        w = np.zeros(n, dtype=np.float32)
        w[1::2] = np.tile([1.0, 3.0], n // 4)  # zero on half the points, uneven on the rest
    observed, expected = np.zeros(n), np.zeros(n)
    firsts = set()
    for seed in range(1, trials + 1):
        (first, second), _ = oracle.kmeans_seed_rows(x, 2, "KMeansPlusPlus", seed, sample_weights=w)
        p = (x[:, 0].astype(np.float64) - float(x[first, 0])) ** 2 * (1.0 if w is None else w.astype(np.float64))
        expected += p / p.sum()  # conditional on the first seed, which ignores the weights
        observed[second] += 1
        firsts.add(first)
    assert len(firsts) == n  # the first seed ranges over every row, zero-weight ones included
    cells = expected > 0
    assert (observed[~cells] == 0).all()  # a zero-weight row is never drawn
    assert cells.sum() == (n // 2 if weighted else n) and expected[cells].min() > 5
    stat = float(((observed[cells] - expected[cells]) ** 2 / expected[cells]).sum())
    dof = int(cells.sum()) - 1
    print(f"chi-square {stat:.1f} at {dof} degrees of freedom, accept below {_chi2_quantile(dof):.1f}")
    assert stat < _chi2_quantile(dof)


def test_the_race_does_not_draw_uniformly():
    # the same statistic against a uniform draw must fail: the test above can tell the two apart
    n, trials = 32, 3000
    x = np.arange(n, dtype=np.float32)[:, None]
    observed = np.zeros(n)
    for seed in range(1, trials + 1):
        observed[oracle.kmeans_seed_rows(x, 2, "KMeansPlusPlus", seed)[0][1]] += 1
    uniform = np.full(n, trials / n)
    assert float(((observed - uniform) ** 2 / uniform).sum()) > _chi2_quantile(n - 1)


def test_forced_rows_replace_the_twins_own_picks():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((300, 4)).astype(np.float32)
    seed = oracle.kmeans_trial_seeds(1)[0]
    ids, steps = oracle.kmeans_seed_rows(x, 6, "KMeansPlusPlus", seed)
    assert len(ids) == 6 and len(set(ids)) == 6 and len(steps) == 5
    assert [s["used"] for s in steps] == ids[1:] == [s["pick"] for s in steps]
    assert all(s["best"] > s["second"] >= 0 for s in steps)
    same, _ = oracle.kmeans_seed_rows(x, 6, "KMeansPlusPlus", seed, forced=ids)
    assert same == ids
    other = [ids[0], (ids[1] + 1) % 300]
    forced_ids, forced_steps = oracle.kmeans_seed_rows(x, 6, "KMeansPlusPlus", seed, forced=other)
    assert forced_ids[:2] == other and forced_steps[0]["pick"] == ids[1]  # the trace still says what the twin wanted
    assert forced_steps[0]["used"] == other[1]


def test_trace_leaves_the_lloyd_results_unchanged():
    rng = np.random.default_rng(7)
    centres = rng.uniform(-3, 3, size=(5, 4))
    x = (centres[rng.integers(0, 5, 800)] + rng.standard_normal((800, 4))).astype(np.float32)
    init = x[:5].copy()
    w = rng.integers(0, 4, 800).astype(np.float32)
    for tol, weights, max_iter in ((1e-2, None, 100), (1e-9, None, 100), (1e-9, w, 100), (1e-9, None, 2)):
        c, lab, inertia, n_iter = oracle.kmeans_lloyd(x, init, max_iter, tol, sample_weights=weights)
        tc, tlab, tinertia, tn_iter, steps = oracle.kmeans_lloyd(x, init, max_iter, tol, sample_weights=weights,
                                                                  trace=True)
        assert (tc == c).all() and (tlab == lab).all() and tinertia == inertia and tn_iter == n_iter
        assert len(steps) == n_iter and steps[0]["ratio"] is None
        assert all(not (s["by_ratio"] or s["by_shift"]) for s in steps[:-1])
        assert (steps[-1]["by_ratio"] or steps[-1]["by_shift"]) == (n_iter < max_iter)
        costs = [s["cost"] for s in steps]
        assert all(b <= a * (1 + 1e-12) for a, b in zip(costs, costs[1:]))  # Lloyd never raises the cost


def test_the_margin_check_rejects_decisions_that_rounding_could_flip():
    def step(ratio, shift):
        return {"ratio": None if ratio is None else float(np.float32(ratio)), "ratio64": ratio, "shift": shift}

    clear = [step(None, 5.0), step(0.9, 1.0), step(0.9995, 0.0)]  # the last one stops by its shift alone
    assert oracle.kmeans_lloyd_margin(clear, 1e-2, 8) and oracle.kmeans_lloyd_margin(clear, 1e-9, 8)
    assert not oracle.kmeans_lloyd_margin([step(None, 5.0), step(0.9895, 1.0)], 1e-2, 8)  # ratio 5e-4 from 0.99
    assert oracle.kmeans_lloyd_margin([step(None, 5.0), step(0.9885, 1.0)], 1e-2, 8)
    assert not oracle.kmeans_lloyd_margin([step(None, 5.0), step(0.9, 1.5e-2)], 1e-2, 8)  # shift within 2x of tol
    assert oracle.kmeans_lloyd_margin([step(None, 5.0), step(0.9, 0.4e-2)], 1e-2, 8)
    # tol below the float32 epsilon: the threshold is 1.0f, the ratio must stay 2 (dim + 2) 2^-24 below 1
    assert not oracle.kmeans_lloyd_margin([step(None, 5.0), step(1.0 - 1e-6, 1.0)], 1e-9, 8)
    assert oracle.kmeans_lloyd_margin([step(None, 5.0), step(1.0 - 2e-6, 1.0)], 1e-9, 8)

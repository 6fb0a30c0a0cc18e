"""CPU: the numpy twin of the ScaNN build (tests/scann_ref.py) against fp64 restatements of the papers' formulas, the C and C++
headers and the exported symbols, and the host-only file writer under the sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import scann_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, U64 = 2.0 ** -24, 2.0 ** -53
ids = lambda c: "x".join(map(str, c))  # noqa: E731


def partition(x, n_leaves, seed):
    """(labels, centres): n_leaves rows as seeds, every row with its nearest seed, centres = the fp32 member means (a leaf with one
    member has its row as its centre: a zero residual)"""
    rng = np.random.default_rng(seed)
    seeds = x[rng.choice(len(x), n_leaves, replace=False)]
    labels = R.nearest_labels(x, seeds)
    centers, _ = R.avq_means_chain32(x, labels, seeds)
    return labels, centers


# ---------------------------------------------------------------------------------------------- 1. headers and exports
def declared_symbols():
    text = open(os.path.join(ROOT, "include", "cuvs_amd", "scann.h")).read()
    return sorted(set(re.findall(r"cuvsError_t\s+(cuvsAmdScann\w+)\(", text)))


def test_header_is_c99_and_symbols_are_exported(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include <cuvs_amd/scann.h>\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    names = declared_symbols()
    assert len(names) == 22 and {"cuvsAmdScannBuild", "cuvsAmdScannSerialize", "cuvsAmdScannAvqCenters", "cuvsAmdScannSoarLabels",
                                 "cuvsAmdScannQuantizeBf16"} <= set(names)
    from cuvs_amd._lib import lib

    assert all(hasattr(lib(), s) for s in names)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "cuvs_amd", "libcuvs_c.so")], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(names) <= exported
    from cuvs_amd.neighbors import scann

    assert all(hasattr(scann, f) for f in ("IndexParams", "Index", "build", "save", "avq_centers", "soar_labels", "quantize_bf16"))


def test_cpp_header_compiles(tmp_path):
    src = tmp_path / "w.cpp"
    src.write_text(
        "#include <cuvs_amd/neighbors.hpp>\n"
        "namespace sc = cuvs::neighbors::experimental::scann;\n"
        "int64_t f(const cuvs::resources& r, cuvs::device_matrix_view<const float> x, cuvs::device_matrix_view<float> c, const uint32_t* l,\n"
        "          uint32_t* o, cuvs::device_matrix_view<int16_t> b) {\n"
        "  sc::index_params p;\n"
        "  p.n_leaves = 32; p.reordering_bf16 = true;\n"
        "  sc::index idx = sc::build(r, p, x);\n"
        "  sc::index host = sc::build(r, p, cuvs::make_host_matrix_view(x.ptr, x.rows, x.cols));\n"
        "  sc::serialize(r, \"dir\", idx);\n"
        "  sc::avq_centers(r, x, l, c, 2.0f);\n"
        "  sc::soar_labels(r, x, cuvs::device_matrix_view<const float>{c.ptr, c.rows, c.cols, false}, l, 1.0f, o);\n"
        "  sc::quantize_bf16(r, x, 0.2f, b);\n"
        "  return idx.size() + idx.dim() + idx.n_leaves() + idx.pq_dim() + idx.pq_bits() + idx.centers().rows + idx.labels().rows +\n"
        "         idx.soar_labels().rows + idx.pq_codebook().rows + idx.quantized_residuals().rows + idx.quantized_soar_residuals().rows +\n"
        "         idx.bf16_dataset().rows + host.size();\n"
        "}\nint main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


# ---------------------------------------------------------------------------------------------- 2. AVQ twin
AVQ_CASES = [(2000, 64, 16), (300, 18, 5)]


@pytest.mark.parametrize("case", AVQ_CASES, ids=ids)
def test_avq_eta_one_is_plain_kmeans(case):
    n, dim, n_leaves = case
    x = R.uniform(n, dim, n + dim)
    labels, centers = partition(x, n_leaves, 1)
    out, r, raw, _ = R.avq_centers(x, labels, np.zeros_like(centers), 1.0)
    means = np.stack([x[labels == c].astype(np.float64).mean(0) for c in range(n_leaves)])
    assert np.abs(raw - means).max() <= 4 * U64 * np.abs(means).max()
    assert abs(r - 1.0) <= 8 * dim * U64
    # the fp32 chain of the device: the means to fp32 rounding of a sequential sum, the rescale 1 to fp32 rounding
    out32, r32 = R.avq_means_chain32(x, labels, np.zeros_like(centers))
    biggest = max(int((labels == c).sum()) for c in range(n_leaves))
    assert np.abs(out32 - means).max() <= (biggest + 4) * U32 * np.abs(means).max()
    assert abs(float(r32) - 1.0) <= 4 * U32


@pytest.mark.parametrize("eta", [0.5, 2.0, 4.0])
@pytest.mark.parametrize("case", AVQ_CASES, ids=ids)
def test_avq_centres_are_stationary_points_of_the_loss(case, eta):
    """Checks the formula, not the code: at c = eta inverse(A) b the gradient of sum_i w1_i (eta |r_par|^2 + |r_perp|^2) is zero.
    A solve with condition number k leaves a relative residual of about dim k 2^-53, and summing n_c terms adds n_c 2^-53 of
    their mass: the bound is (n_c + 8 dim k) 2^-53 times the sum of the absolute terms. The condition number stays under
    max(eta, 1 / eta) because trace(sum w3 x x^T) = S."""
    n, dim, n_leaves = case
    x = R.uniform(n, dim, n + dim)
    labels, centers = partition(x, n_leaves, 1)
    out, r, raw, conds = R.avq_centers(x, labels, centers, eta)
    kappa = max(eta, 1.0 / eta)
    print(case, eta, "rescale", r, "largest condition number", max(conds))
    assert max(conds) <= kappa * (1 + 1e-9) and min(conds) >= 1.0 - 1e-9
    worst = 0.0
    for c in range(n_leaves):
        g, mass = R.avq_gradient(x, labels, raw, eta, c)
        n_c = int((labels == c).sum())
        worst = max(worst, float((np.abs(g) / mass).max()))
        assert (np.abs(g) <= (n_c + 8 * dim * kappa) * U64 * mass).all()
    print("largest |gradient| / mass", worst)
    assert 0.5 < r < 2.0 and np.allclose(out, raw * r, rtol=1e-15)
    # the fp32 restatement stays within the error of an fp32 solve
    out32, _, _, _ = R.avq_centers(x, labels, centers, eta, np.float32)
    err = np.abs(out32.astype(np.float64) - out).max()
    print("fp32 restatement against fp64:", err)
    assert err <= 4 * dim * kappa * U32 * np.abs(out).max()


def test_avq_edge_rules():
    x = R.uniform(40, 6, 3)
    x[5] = 0  # a zero row: weights 0
    labels = (np.arange(40) % 4).astype(np.int32)
    labels[labels == 2] = 1  # leaf 2 is empty
    k = R.uniform(5, 6, 4)  # leaf 4 is empty too
    for eta in (1.0, 2.0):
        out, r, raw, _ = R.avq_centers(x, labels, k, eta)
        assert (out[2] == k[2]).all() and (out[4] == k[4]).all()  # kept, and not rescaled
        keep = np.arange(40) != 5
        out2, r2, _, _ = R.avq_centers(x[keep], labels[keep], k, eta)
        # the zero row moves no centre; it only counts in n_c of the rescale's denominator
        assert np.allclose(raw, R.avq_centers(x[keep], labels[keep], k, eta)[2], rtol=1e-13)
        assert r < r2 if eta == 1.0 else True
    # all rows zero: nothing is updated, the denominator is 0, rescale is 1
    out, r, _, _ = R.avq_centers(np.zeros((8, 3), np.float32), np.zeros(8, np.int32), k[:1, :3], 2.0)
    assert r == 1.0 and (out == k[:1, :3]).all()


# ---------------------------------------------------------------------------------------------- 3. SOAR twin
SOAR_CASES = [(1000, 18, 33, 7), (777, 67, 130, 11)]  # rows, dim, leaves, seed (the seeds were kept after running: see the test)


def soar_bound(x, centers, labels, lam, j):
    """The fp32 score of (row i, centre j[i]) against its exact value, u = 2^-24, first order. A chain of length d errs by at most
    d u sum|u_k v_k|. rh_k carries (d / 2 + 3) u relatively (the subtraction, the chain and the root of nr, the division), so
    a_j and p err by (1.5 d + 3) u (A_j + P), A_j = sum|rh_k c_jk|, P = sum|rh_k x_k|, and t = a_j - p by that plus u |t|;
    lambda t^2 moves by 2 lambda |t| times that, plus its own two roundings. b_j and cn_j err by d u B_j and d u cn_j,
    B_j = sum|x_k c_jk|, and the three outer operations add u times the partial results. In all, generously:
    E = u ((3 d + 8) lambda |t| (A_j + P) + (d + 4) (lambda t^2 + 2 B_j + cn_j))."""
    x64, c64 = x.astype(np.float64), centers.astype(np.float64)
    d = x.shape[1]
    r = x64 - c64[labels]
    nr = np.sqrt((r * r).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        rh = np.where(nr[:, None] == 0, 0.0, r / nr[:, None])
    cj = c64[j]
    t = (rh * cj).sum(1) - (rh * x64).sum(1)
    A, P, B, cn = (np.abs(rh) * np.abs(cj)).sum(1), (np.abs(rh) * np.abs(x64)).sum(1), (np.abs(x64) * np.abs(cj)).sum(1), (cj * cj).sum(1)
    return U32 * ((3 * d + 8) * lam * np.abs(t) * (A + P) + (d + 4) * (lam * t * t + 2 * B + cn))


@pytest.mark.parametrize("lam", [0.0, 1.0, 1.5])
@pytest.mark.parametrize("case", SOAR_CASES, ids=ids)
def test_soar_twin_against_fp64(case, lam):
    """The expanded fp32 form against the fp64 argmin of |r'|^2 + lambda <rh, r'>^2. With these seeds the labels agree on every row
    (seeds 0 .. 12 were run: all agree at both shapes but for single near-ties); the test allows 1 % of the rows to differ, each
    within the bound of soar_bound for both centres."""
    n, dim, n_leaves, seed = case
    x = R.uniform(n, dim, seed)
    labels, centers = partition(x, n_leaves, seed)
    got = R.soar_labels(x, centers, labels, lam)
    s64 = R.soar_scores64(x, centers, labels, lam)
    want = s64.argmin(1)
    differ = np.flatnonzero(got != want)
    same_leaf = float((got == labels).mean())
    print(case, lam, "rows that differ from fp64:", len(differ), "rows whose SOAR leaf is their primary leaf: %.1f %%" % (100 * same_leaf))
    assert len(differ) <= n // 100
    rows = np.arange(n)
    gap = s64[rows, got] - s64[rows, want]
    bound = soar_bound(x, centers, labels, lam, got) + soar_bound(x, centers, labels, lam, want)
    assert (gap[differ] <= bound[differ]).all()
    assert got.min() >= 0 and got.max() < n_leaves
    if n == 777:  # singleton leaves: zero residuals, the reference divides by zero there
        _, nr = R.soar_scores(x, centers, labels, lam)
        zero = np.flatnonzero(nr == 0)
        assert len(zero) > 0 and np.isfinite(R.soar_scores(x[zero], centers, labels[zero], lam)[0]).all()
        assert (got[zero] == want[zero]).all()


def test_soar_ties_go_to_the_lower_id():
    x = R.uniform(50, 6, 5)
    labels, centers = partition(x, 4, 5)
    centers = np.concatenate([centers, centers[1:3]])  # centres 4 and 5 repeat 1 and 2
    got = R.soar_labels(x, centers, labels, 1.0)
    assert not np.isin(got, (4, 5)).any() and np.isin(got, (1, 2)).any()


# ---------------------------------------------------------------------------------------------- 4. bf16 twin
def special_rows():
    rng = np.random.default_rng(9)
    x = rng.uniform(-2, 2, (12, 24)).astype(np.float32)
    x[0] = 0                                   # a zero row
    x[1] = x[1] * np.float32(0.2 / 8) / np.sqrt((x[1].astype(np.float64) ** 2).sum()).astype(np.float32)  # |x| well below T
    x[2, :8] = R.bf16_value(R.bf16_rne_bits(x[2, :8]))  # coordinates that are exact in bf16
    x[3] = -np.abs(x[3])                       # negative coordinates
    x[4, 0] = np.float32(1.0) - np.float32(2.0 ** -10)  # rounds up to 1.0: the neighbour below crosses a power of two
    x[4, 1] = np.float32(-2.0) + np.float32(2.0 ** -9)
    x[5, 0] = np.float32(3.3e38)               # rounds to the largest finite bf16 or beyond: no infinite neighbour is taken
    return x


def test_bf16_plain_rounding_is_round_to_nearest_even():
    x = np.concatenate([special_rows().ravel(), R.uniform(4096, 1, 2, -5, 5).ravel(),
                        np.array([1.00390625, 1.01171875, -1.00390625, 0.0, -0.0, 1e-40, 65280.0], np.float32)]).astype(np.float32)[None, :]
    got = R.quantize_bf16(x)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy()  # an independent implementation
    assert got.dtype == np.int16 and (got == want).all()
    assert R.bf16_value(got.view(np.uint16))[0, -7] == 1.0 and R.bf16_value(got.view(np.uint16))[0, -6] == 1.015625  # ties to even


@pytest.mark.parametrize("dim", [1, 24, 63, 64, 65, 200])
def test_bf16_noise_shaping_twin(dim):
    T = 0.2
    x = special_rows()[:, :dim] if dim == 24 else R.uniform(40, dim, dim, -2, 2)
    hist = []
    got = R.quantize_bf16(x, T, hist).view(np.uint16)
    plain = R.bf16_rne_bits(x)
    assert (hist[0] == plain).all() and (hist[-1] == got).all() and len(hist) <= R.MAX_ROUNDS + 1
    # every coordinate is one of the two bf16 values bracketing x_d
    q = R.bf16_value(got)
    other, has = R.bf16_neighbor(plain, x)
    assert ((got == plain) | (has & (got == other))).all()
    lo, hi = np.minimum(R.bf16_value(plain), np.where(has, R.bf16_value(other), R.bf16_value(plain))), \
        np.maximum(R.bf16_value(plain), np.where(has, R.bf16_value(other), R.bf16_value(plain)))
    assert ((lo <= x) & (x <= hi) | ~has).all() and np.isfinite(q).all()
    # the loss never rises from round to round and ends no higher than plain rounding's; the slack is the rounding error of this
    # test's own fp64 evaluation (|r|^2 - |r_par|^2 cancels completely at dim 1, where eta_x = 0): (dim + 4) 2^-53 of the terms
    both = [R.avq_row_loss(x, h, T) for h in hist]
    loss, mass = [b[0] for b in both], [b[1] for b in both]
    for t in range(len(loss) - 1):
        assert (loss[t + 1] <= loss[t] + (dim + 4) * U64 * (mass[t] + mass[t + 1])).all()
    assert (loss[-1] <= loss[0] + (dim + 4) * U64 * (mass[0] + mass[-1])).all()
    moved = (got != plain).any(1)
    print("dim", dim, "rounds", len(hist) - 1, "rows moved", int(moved.sum()), "loss ratio", float(loss[-1].sum() / loss[0].sum()))
    sq = (x.astype(np.float64) ** 2).sum(1)
    assert not moved[sq <= T * T].any()
    if dim >= 63:
        assert moved.sum() > len(x) // 2 and loss[-1].sum() < loss[0].sum()
    if dim == 24:
        assert not moved[0] and not moved[1]                 # the zero row, the row with |x| <= T
        assert (got[2, :8] == plain[2, :8]).all()            # exact coordinates have no candidate
        assert (q[3] <= 0).all() and moved[3]                # negative coordinates stay negative, and do move
        assert set(q[4, :2]) <= {1.0, 0.99609375, -2.0, -1.9921875}
        assert np.isfinite(q[5, 0])


# ---------------------------------------------------------------------------------------------- 5. the file writer
@pytest.mark.parametrize("bits,bf16", [(8, True), (4, False)])
def test_file_writer_under_the_sanitizers(tmp_path, bits, bf16):
    exe = tmp_path / "scann_host_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "cuvs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "scann_host_test.cpp"), "-o", str(exe)])
    n, dim, n_leaves, pq_dim = 300, 6, 7, 2  # three subspaces: the odd nibble at 4 bits
    n_sub, book_n = dim // pq_dim, 1 << bits
    x = R.uniform(n, dim, 21)
    labels, centers = partition(x, n_leaves, 21)
    soar = R.soar_labels(x, centers, labels, 1.0)
    assert (soar == labels).any() and (soar != labels).any()
    rng = np.random.default_rng(4)
    codebook = rng.normal(0, 1, (book_n, dim)).astype(np.float32)
    codes = rng.integers(0, book_n, (n, n_sub)).astype(np.uint8)
    soar_codes = rng.integers(0, book_n, (n, n_sub)).astype(np.uint8)

    def pack(c):
        if bits == 8:
            return c
        out = np.zeros((n, (n_sub * 4 + 7) // 8), np.uint8)
        for j in range(n_sub):
            out[:, j // 2] |= (c[:, j] << (4 * (j % 2))).astype(np.uint8)
        return out

    bf = R.quantize_bf16(x, 0.2)
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    dst.mkdir()
    for name, a in (("centers.f32", centers), ("labels.u32", labels.astype(np.uint32)), ("soar.u32", soar.astype(np.uint32)),
                    ("codebook.f32", codebook), ("codes.u8", pack(codes)), ("soar_codes.u8", pack(soar_codes)), ("bf16.i16", bf)):
        np.ascontiguousarray(a).tofile(str(src / name))
    out = subprocess.run([str(exe), str(src), str(dst), str(n), str(dim), str(n_leaves), str(pq_dim), str(bits), str(int(bf16))],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "scann host OK" in out.stdout
    meta = R.read_metadata(str(dst / "cuvs_metadata.bin"))
    assert [m.dtype for m in meta] == [np.int32, np.uint32, np.uint32] and [int(m) for m in meta] == [1, dim, pq_dim]
    assert all(m.shape == () for m in meta)
    load = lambda name: np.load(str(dst / name))  # noqa: E731
    c = load("centers.npy")
    assert c.dtype == np.float32 and (c == centers).all()
    t = load("datapoint_to_token.npy")
    assert t.dtype == np.int32 and t.shape == (2 * n,) and (t == R.interleave_labels(labels, soar)).all()
    assert (t[1::2] == -1).sum() == (soar == labels).sum() > 0
    b = load("pq_codebook.npy")
    assert b.dtype == np.float32 and b.shape == (book_n, dim) and (b == codebook).all()
    for name, want in (("hashed_dataset.npy", codes), ("hashed_dataset_soar.npy", soar_codes)):
        h = load(name)
        assert h.dtype == np.uint8 and h.shape == (n, n_sub) and (h == want).all()
    if bf16:
        q = load("bf16_dataset.npy")
        assert q.dtype == np.int16 and (q == bf).all()
    else:
        assert not (dst / "bf16_dataset.npy").exists()
    assert sorted(os.listdir(dst)) == sorted(["cuvs_metadata.bin", "centers.npy", "datapoint_to_token.npy", "pq_codebook.npy",
                                              "hashed_dataset.npy", "hashed_dataset_soar.npy"] + (["bf16_dataset.npy"] if bf16 else []))

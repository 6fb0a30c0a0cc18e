"""CPU: the numpy twin of the epsilon-neighbourhood search against scipy, the C header and the exported symbols, the host-only
helper under the sanitizers, and the blob inputs of the reference table."""
import json
import os
import subprocess

import numpy as np

from tests import eps_neighbors_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "eps_neighbors_reference_table.json")
EXPORTS = ["cuvsAmdEpsNeighbors", "cuvsAmdEpsNeighborsCsr", "cuvsAmdEpsNeighborsLastStats"]


def test_twin_against_scipy():
    from scipy.spatial.distance import cdist

    rng = np.random.default_rng(7)
    x = rng.random((96, 24)).astype(np.float32)
    y = rng.random((500, 24)).astype(np.float32)
    d64 = cdist(x.astype(np.float64), y.astype(np.float64), "sqeuclidean")
    eps = np.float32(np.median(d64))
    clear = np.abs(d64 - np.float64(eps)) > 1e-5 * np.float64(eps)
    assert clear.sum() > clear.size // 2, "the comparison would be vacuous"
    adj = R.member(R.chain(x, y), eps)
    assert (adj[clear] == (d64 <= np.float64(eps))[clear]).all()
    assert 0.3 < adj.mean() < 0.7
    # the protocols derived from the membership matrix
    vd = R.degrees(adj)
    indptr, indices = R.csr_of(adj)
    assert vd[-1] == adj.sum() == indptr[-1] == len(indices) and (np.diff(indptr) == vd[:-1]).all()
    indptr2, indices2 = R.csr_of(adj, max_k=3)
    assert (np.diff(indptr2) == np.minimum(vd[:-1], 3)).all() and (indices2[:3] == indices[:3]).all()


def test_twin_edge_cases():
    kat = R.int_kat(1)
    acc = R.chain(kat, kat)
    assert (acc == np.rint(acc)).all() and acc.max() <= 32
    adj = R.member(acc, 6.0)
    assert int((acc == 6).sum()) == 884 and int(adj.sum()) == 2936  # pairs on the radius count as inside
    assert not R.member(acc, -1.0).any()
    assert R.member(R.chain(kat[:, :0], kat[:, :0]), 0.0).all()  # dim == 0: 0 <= eps
    nan = kat.copy()
    nan[3, 2] = np.nan
    assert not R.member(R.chain(nan, kat), 1e30)[3].any() and R.member(R.chain(nan, kat), 1e30)[4].all()


def test_spheres_sit_on_the_radius():
    x, y, eps, acc, adj = R.spheres_twin(64, 4096, 16, 16)
    own = acc[np.arange(4096) % 64, np.arange(4096)]
    ulp = np.spacing(eps)
    assert (np.abs(own.astype(np.float64) - np.float64(eps)) <= 8 * ulp).all()
    assert 0.3 < adj[np.arange(4096) % 64, np.arange(4096)].mean() < 0.7
    # another arithmetic flips pairs: the expanded form in fp32
    xx = (x * x).sum(axis=1, dtype=np.float32)
    yy = (y * y).sum(axis=1, dtype=np.float32)
    expanded = (xx[:, None] + yy[None, :] - np.float32(2) * (x @ y.T)).astype(np.float32)
    assert ((expanded <= eps) != adj).sum() > 100


def test_header_is_c99_and_symbols_are_exported(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include <cuvs_amd/eps_neighbors.h>\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    from cuvs_amd._lib import lib

    assert all(hasattr(lib(), s) for s in EXPORTS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "cuvs_amd", "libcuvs_c.so")], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(EXPORTS) <= names


def test_cpp_wrappers_compile(tmp_path):
    src = tmp_path / "w.cpp"
    src.write_text(
        "#include <cuvs_amd/neighbors.hpp>\n"
        "namespace en = cuvs_amd::neighbors::epsilon_neighborhood;\n"
        "struct half_t { unsigned short bits; };  // any 2-byte element type goes as fp16\n"
        "void f(const cuvs::resources& r, cuvs::device_matrix_view<const float> x, cuvs::device_matrix_view<const half_t> h,\n"
        "       cuvs::device_matrix_view<bool> adj, int64_t* v64, int32_t* v32, float* d, int64_t* max_k) {\n"
        "  en::compute(r, x, x, adj, v64, 4.f);\n"
        "  en::compute(r, h, h, adj, v32, 4.f, L2Unexpanded);\n"
        "  en::csr(r, x, x, v64, (int64_t*)nullptr, (float*)nullptr, 0, v64, 4.f);\n"
        "  en::csr(r, h, h, v64, v64, d, 100, (int64_t*)nullptr, 4.f, max_k);\n"
        "}\nint main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_host_helper_under_the_sanitizers(tmp_path):
    exe = tmp_path / "eps_neighbors_host_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "cuvs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "eps_neighbors_host_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "eps neighbors host OK" in out.stdout


def test_reference_table_blobs_have_exact_degrees():
    table = json.load(open(TABLE))
    assert len(table["inputsfi"]["rows"]) == 14 and len(table["inputsfi_rbc"]["rows"]) == 14
    run = [r for r in table["inputsfi"]["rows"] + table["inputsfi_rbc"]["rows"] if r["run"]]
    assert len(run) == 15
    assert [r for r in table["inputsfi"]["rows"] if r["run"]] == [dict(line=87, n_row=15000, n_col=17, n_centers=5, n_batches=1, eps=2.0, run=True)]
    assert sum(1 for r in table["inputsfi"]["rows"] if r["n_col"] == 10000 and not r["run"]) == 2
    smallest = np.inf
    for r in run:
        assert r["n_row"] % r["n_centers"] == 0 and r["n_row"] % r["n_batches"] == 0
        rows, labels, centers = R.blobs(r["n_row"], r["n_col"], r["n_centers"], 1000 * r["n_row"] + r["n_col"])
        assert rows.dtype == np.float32 and (np.bincount(labels) == r["n_row"] // r["n_centers"]).all()
        gap = R.min_center_distance(centers)
        smallest = min(smallest, gap)
        # rows of one centre are closer than eps, rows of two centres further: the degree is exactly the blob size
        spread = np.linalg.norm(rows.astype(np.float64) - centers[labels], axis=1).max()
        assert gap > 2 * r["eps"] and 2 * spread < r["eps"] and gap - 2 * spread > r["eps"], r
    assert smallest > 4.0

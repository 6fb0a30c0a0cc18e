"""CPU: the header of the ScaNN search (C99, exports, the C++ declarations), the twin's own rules on hand-made cases, and the
host-only list builder under the sanitizers."""
import os
import subprocess

import numpy as np
import pytest

from tests import scann_search_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cuvsAmdScannSearchParamsCreate", "cuvsAmdScannSearchParamsDestroy", "cuvsAmdScannSearch", "cuvsAmdScannSearchLastStats"]


def test_header_is_c99_and_symbols_are_exported(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include <cuvs_amd/scann_search.h>\nint main(void) { struct cuvsAmdScannSearchParams p = {20, 0}; return (int)p.n_reorder; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "cuvs_amd", "libcuvs_c.so")], text=True)
    assert set(NAMES) <= {line.split()[-1] for line in out.splitlines() if line.strip()}
    from cuvs_amd.neighbors import scann

    assert all(hasattr(scann, f) for f in ("SearchParams", "search", "search_last_stats"))


def test_cpp_declarations_compile(tmp_path):
    src = tmp_path / "w.cpp"
    src.write_text(
        "#include <cuvs_amd/neighbors.hpp>\n"
        "namespace sc = cuvs::neighbors::experimental::scann;\n"
        "uint64_t f(const cuvs::resources& r, const sc::index& idx, cuvs::device_matrix_view<const float> q,\n"
        "           cuvs::device_matrix_view<int64_t> n, cuvs::device_matrix_view<float> d) {\n"
        "  sc::search_params p;\n"
        "  p.n_probes = 8; p.n_reorder = 100;\n"
        "  sc::search(r, p, idx, q, n, d);\n"
        "  return sc::search_last_stats()[3];\n"
        "}\nint main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def tiny_index():
    """5 rows in 2 leaves and 1 dimension: row 1 sits in both leaves, and its SOAR codes reproduce it better than its primary ones"""
    return dict(centers=np.array([[0.0], [4.0]], np.float32), labels=np.array([0, 0, 1, 1, 0], np.uint32),
                soar_labels=np.array([0, 1, 1, 1, 0], np.uint32), pq_codebook=np.array([[0.0], [1.0], [-2.0], [0.5]], np.float32),
                codes=np.array([[0], [0], [0], [1], [3]], np.uint8), soar_codes=np.array([[0], [2], [0], [1], [3]], np.uint8))


def test_twin_lists_t_and_dedupe():
    a = tiny_index()
    rows, leaf, codes = S.lists(a)
    assert rows.tolist() == [0, 1, 4, 1, 2, 3] and leaf.tolist() == [0, 0, 0, 1, 1, 1] and codes.ravel().tolist() == [0, 0, 3, 2, 0, 1]
    rt = S.decode(a["pq_codebook"], codes, 1)
    # t = 2 <centre, r~> + |r~|^2: |q - (c + r~)|^2 = |q - c|^2 + t - 2 <q, r~>
    assert S.entry_t(a["centers"], leaf, rt).tolist() == [0.0, 0.0, 0.25, 2 * 4 * -2 + 4, 0.0, 2 * 4 + 1]
    q = np.array([[2.0]], np.float32)  # row 1 is 2.0 = 4 - 2 through its SOAR entry, 0.0 through its primary one
    _, _, score, tol = S.entry_scores(q, a, S.L2, 1)
    assert score[0].tolist() == [4.0, 4.0, 2.25, 0.0, 4.0, 9.0] and (tol > 0).all()
    best, _ = S.row_scores(rows, score, tol, 5)
    assert best[0].tolist() == [4.0, 0.0, 4.0, 9.0, 2.25]
    # the rule: the best min(2 m, available) entries by (score, row), first occurrences, the first m
    assert S.dedupe(rows, score[0], 3)[0].tolist() == [1, 4, 0]          # 6 entries: row 1's second entry is dropped
    assert S.dedupe(rows, score[0], 2)[0].tolist() == [1, 4]             # 4 entries: (1, 4, 0, 1) -> 1, 4
    assert S.dedupe(rows, score[0], 5)[0].tolist() == [1, 4, 0, 2, 3]    # fewer entries than 2 m
    _, _, ip, _ = S.entry_scores(q, a, S.IP, 1)
    assert ip[0].tolist() == [0.0, 0.0, 1.0, 8.0 - 4.0, 8.0, 10.0]        # <q, c> + <q, r~>


@pytest.mark.parametrize("shape", [(300, 18, 7, 3, 8), (257, 6, 5, 2, 4), (100, 40, 3, 8, 4)], ids=lambda s: "x".join(map(str, s)))
def test_list_builder_under_the_sanitizers(tmp_path, shape):
    exe = tmp_path / "scann_search_host_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "cuvs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "scann_search_host_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)] + [str(v) for v in shape], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "scann search host OK" in out.stdout, out.stdout + out.stderr

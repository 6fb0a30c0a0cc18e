"""CPU: the C header, the exported symbols, the C++ wrappers and the Python names of the exact Hamming kNN."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ["cuvsAmdBinaryKnn", "cuvsAmdBinaryPairwiseDistance", "cuvsAmdBinaryKnnLastStats"]


def test_header_is_c99_and_symbols_are_exported(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include <cuvs_amd/binary_knn.h>\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "cuvs_amd", "libcuvs_c.so")], text=True)
    assert set(EXPORTS) <= {line.split()[-1] for line in out.splitlines() if line.strip()}
    import cuvs_amd

    assert all(hasattr(cuvs_amd.neighbors.binary_brute_force, f) for f in ("knn", "pairwise_distance", "last_stats"))


def test_cpp_wrappers_compile(tmp_path):
    src = tmp_path / "w.cpp"
    src.write_text(
        "#include <cuvs_amd/binary_knn.hpp>\n"
        "namespace bbf = cuvs::neighbors::binary_brute_force;\n"
        "void f(const cuvs::resources& r, cuvs::device_matrix_view<const uint8_t> x, cuvs::device_matrix_view<const int8_t> s,\n"
        "       cuvs::device_matrix_view<int64_t> idx, cuvs::device_matrix_view<float> dist, const uint32_t* words) {\n"
        "  bbf::knn(r, x, x, idx, dist);\n"
        "  bbf::knn(r, s, s, idx, dist, cuvs::neighbors::filtering::bitset_filter{words, x.extent(0)});\n"
        "  bbf::pairwise_distance(r, x, x, dist);\n"
        "}\nint main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])

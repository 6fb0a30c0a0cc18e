"""CPU: the C header, the exported symbols, the C++ wrappers and the Python names of the masked nearest neighbour."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ["cuvsAmdMaskedL2NN", "cuvsAmdCrossComponentNN", "cuvsAmdMaskedNNLastStats"]


def test_header_is_c99_and_symbols_are_exported(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include <cuvs_amd/masked_nn.h>\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "cuvs_amd", "libcuvs_c.so")], text=True)
    assert set(EXPORTS) <= {line.split()[-1] for line in out.splitlines() if line.strip()}
    import cuvs_amd

    assert all(hasattr(cuvs_amd.distance, f) for f in ("masked_l2_nn", "cross_component_nn"))


def test_cpp_wrappers_compile(tmp_path):
    src = tmp_path / "w.cpp"
    src.write_text(
        "#include <cuvs_amd/distance.hpp>\n"
        "void f(const cuvs::resources& r, cuvs::device_matrix_view<const float> x, cuvs::device_matrix_view<const bool> adj,\n"
        "       const int64_t* ends, const int32_t* colors, int64_t* idx, float* dist) {\n"
        "  cuvs::distance::masked_l2_nn(r, {true, false}, x, x, nullptr, nullptr, adj, ends, idx, dist);\n"
        "  cuvs::neighbors::cross_component_nn(r, x, colors, 3, nullptr, nullptr, idx, idx, dist, true);\n"
        "}\nint main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])

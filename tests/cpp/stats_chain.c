/* Compiled restatement of the three fp32 chains of tests/stats_ref.py for the large shapes of the GPU tests (the numpy chain
 * costs a minute at 2048 x 2048 x 128). Built by stats_ref.py with -ffp-contract=off: only the explicit fmaf calls fuse, and
 * fmaf is correctly rounded. tests/test_stats_cpu.py holds it to the numpy chain bit for bit.
 * mode 0: acc = fmaf(d, d, acc), d = x[i][t] - x[j][t]; 1: acc = acc + fabsf(d); 2: acc = fmaf(x[i][t], x[j][t], acc). */
#include <math.h>
#include <stdint.h>

void stats_chain(const float* x, int64_t n, int64_t dim, int mode, float* out)
{
#pragma omp parallel for schedule(static)
  for (int64_t i = 0; i < n; ++i) {
    const float* a = x + i * dim;
    for (int64_t j = 0; j < n; ++j) {
      const float* b = x + j * dim;
      float acc      = 0.f;
      if (mode == 0) {
        for (int64_t t = 0; t < dim; ++t) {
          const float d = a[t] - b[t];
          acc           = fmaf(d, d, acc);
        }
      } else if (mode == 1) {
        for (int64_t t = 0; t < dim; ++t) acc = acc + fabsf(a[t] - b[t]);
      } else {
        for (int64_t t = 0; t < dim; ++t) acc = fmaf(a[t], b[t], acc);
      }
      out[i * n + j] = acc;
    }
  }
}

/*
 * oracle_nn_descent.c — the pair key of the NN-descent kernels (TEST INFRASTRUCTURE ONLY, see oracle.c).
 *
 * The one piece of tests/nn_descent_ref.py that numpy cannot state: the team arithmetic of
 * cuvs_amd/csrc/nn_descent.hip team_pair_key, whose fused multiply-add rounds once. Rows arrive as floats (fp16, int8
 * and uint8 values are exact in fp32); vl is the number of elements of the row type in 16 bytes (4 / 8 / 16).
 *   lane t of the 8-lane team takes the elements t vl + 8 vl j + e (j = 0, 1, ...; e = 0 .. vl - 1) in that order and
 *   accumulates fmaf((x - y), (x - y), acc) for L2 or fmaf(x, y, acc) otherwise; the 8 partial sums are combined by the
 *   xor butterfly 1, 2, 4; inner product negates; cosine is 1 - acc / (|a| |b|), and 0 when |a| |b| is not positive
 *   (reference detail/nn_descent.cuh:534-537); the float becomes an order-preserving uint32 key.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define EXPORT __attribute__((visibility("default")))

static uint32_t nnd_f2key(float f)
{
  uint32_t u;
  memcpy(&u, &f, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

/* mode: 0 L2, 1 inner product, 2 cosine (norms = |row|, fp32) */
EXPORT void oracle_nnd_pair_keys(const float* x, int64_t dim, int vl, int mode, const float* norms, const uint32_t* a,
                                 const uint32_t* b, int64_t m, uint32_t* keys)
{
#pragma omp parallel for schedule(static)
  for (int64_t i = 0; i < m; ++i) {
    const float* ra = x + (int64_t)a[i] * dim;
    const float* rb = x + (int64_t)b[i] * dim;
    float p[8], q[8];
    for (int t = 0; t < 8; ++t) {
      float acc = 0.f;
      for (int64_t d0 = (int64_t)t * vl; d0 < dim; d0 += 8 * (int64_t)vl)
        for (int e = 0; e < vl && d0 + e < dim; ++e) {
          if (mode == 0) { const float df = ra[d0 + e] - rb[d0 + e]; acc = fmaf(df, df, acc); }
          else           acc = fmaf(ra[d0 + e], rb[d0 + e], acc);
        }
      p[t] = acc;
    }
    for (int s = 1; s < 8; s <<= 1) {
      for (int t = 0; t < 8; ++t) q[t] = p[t] + p[t ^ s];
      memcpy(p, q, sizeof p);
    }
    float d = p[0];
    if (mode == 1) d = -d;
    if (mode == 2) {
      const float np = norms[a[i]] * norms[b[i]];
      d              = np > 0.0f ? 1.0f - d / np : 0.0f;
    }
    keys[i] = nnd_f2key(d);
  }
}

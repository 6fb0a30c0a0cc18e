// Host-only parts of the spectral eigen-solver (spectral.hip): the size of the Lanczos basis, the hashed start
// vector, the projected matrix of a thick-restart cycle (diagonal plus arrow plus tridiagonal), its dense symmetric
// eigen-solver in double (cyclic Jacobi) and the convergence test. No HIP, no DLPack and no LAPACK in here:
// tests/cpp/spectral_host_test.cpp builds this header alone.
#pragma once

#include "mix_hash.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

namespace cuvs_amd {
namespace spectral_host {

constexpr double kEps32 = 1.1920928955078125e-07;  // 2^-23
constexpr int kMaxNcv   = 1024;                    // rows of the basis the re-orthogonalisation kernels stage per workgroup

// the reference's rule (detail/spectral_embedding.cuh:67), raised to k + 1: a restart keeps k vectors and needs one more
inline int64_t ncv_rule(int64_t n, int64_t k)
{
  return std::max<int64_t>(std::min<int64_t>(n - k, std::max<int64_t>(2 * k + 1, 20)), k + 1);
}

// the iteration stops at `tol`, but never above fp32 resolution: a run that stops earlier returns before the copies of a
// multiple eigenvalue, which only rounding brings into the Krylov space, have grown
inline double stop_tolerance(double tol) { return (tol <= 0.0 || tol > kEps32) ? kEps32 : tol; }

// a basis vector whose norm fell to this is rounding noise: the Krylov space is exhausted. `scale` bounds ||L||_inf.
inline double collapse_threshold(double scale) { return 8.0 * kEps32 * scale; }

CUVS_AMD_MIX_HD inline uint32_t seed_fold(uint64_t seed) { return mix_hash((uint32_t)(seed >> 32), (uint32_t)seed); }

// element i of the pseudo-random vector number `salt` (0: the start vector): uniform in [-1, 1), exact in fp32
CUVS_AMD_MIX_HD inline float hashed_uniform(uint32_t fold, uint32_t salt, uint32_t i)
{
  return (float)(mix_hash(fold + salt, i) >> 8) * 1.1920928955078125e-07f - 1.0f;
}

// Eigen-decomposition of the symmetric matrix a [m, m] (row-major, destroyed) by cyclic Jacobi: evals ascending, vecs [m, m]
// row-major with eigenvector i in COLUMN i.
inline void jacobi_eigh(int m, std::vector<double>& a, std::vector<double>& evals, std::vector<double>& vecs)
{
  vecs.assign((size_t)m * m, 0.0);
  for (int i = 0; i < m; ++i) vecs[(size_t)i * m + i] = 1.0;
  double frob = 0.0;
  for (double v : a) frob += v * v;
  frob = std::sqrt(frob);
  for (int sweep = 0; sweep < 100; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < m; ++p)
      for (int q = p + 1; q < m; ++q) off += a[(size_t)p * m + q] * a[(size_t)p * m + q];
    if (std::sqrt(off) <= std::ldexp(frob, -58)) break;
    for (int p = 0; p < m; ++p) {
      for (int q = p + 1; q < m; ++q) {
        const double apq = a[(size_t)p * m + q];
        if (apq == 0.0) continue;
        const double theta = (a[(size_t)q * m + q] - a[(size_t)p * m + p]) / (2.0 * apq);
        const double t     = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int r = 0; r < m; ++r) {  // columns p and q
          const double arp = a[(size_t)r * m + p], arq = a[(size_t)r * m + q];
          a[(size_t)r * m + p] = c * arp - s * arq;
          a[(size_t)r * m + q] = s * arp + c * arq;
        }
        for (int r = 0; r < m; ++r) {  // rows p and q
          const double apr = a[(size_t)p * m + r], aqr = a[(size_t)q * m + r];
          a[(size_t)p * m + r] = c * apr - s * aqr;
          a[(size_t)q * m + r] = s * apr + c * aqr;
        }
        a[(size_t)p * m + q] = 0.0;
        a[(size_t)q * m + p] = 0.0;
        for (int r = 0; r < m; ++r) {
          const double vrp = vecs[(size_t)r * m + p], vrq = vecs[(size_t)r * m + q];
          vecs[(size_t)r * m + p] = c * vrp - s * vrq;
          vecs[(size_t)r * m + q] = s * vrp + c * vrq;
        }
      }
    }
  }
  std::vector<int> order((size_t)m);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return a[(size_t)x * m + x] < a[(size_t)y * m + y]; });
  evals.resize((size_t)m);
  std::vector<double> sorted((size_t)m * m);
  for (int i = 0; i < m; ++i) {
    evals[(size_t)i] = a[(size_t)order[i] * m + order[i]];
    for (int r = 0; r < m; ++r) sorted[(size_t)r * m + i] = vecs[(size_t)r * m + order[i]];
  }
  vecs.swap(sorted);
}

// the projected matrix of a cycle: theta[i] on the diagonal and arrow[i] in row and column `locked` for i < locked, then
// alpha[j] on the diagonal and beta[j + 1] beside it for locked <= j < m
inline std::vector<double> projected_matrix(int m, int locked, const double* theta, const double* arrow, const double* alpha,
                                            const double* beta)
{
  std::vector<double> t((size_t)m * m, 0.0);
  for (int i = 0; i < locked && i < m; ++i) {
    t[(size_t)i * m + i] = theta[i];
    if (locked < m) t[(size_t)i * m + locked] = t[(size_t)locked * m + i] = arrow[i];
  }
  for (int j = locked; j < m; ++j) {
    t[(size_t)j * m + j] = alpha[j];
    if (j + 1 < m) t[(size_t)j * m + j + 1] = t[(size_t)(j + 1) * m + j] = beta[j + 1];
  }
  return t;
}

// what the host decides at the end of a cycle
struct cycle {
  int m_eff      = 0;      // order of the projected problem: the steps before a collapsed vector
  bool collapsed = false;  // a basis vector was rounding noise: the next cycle starts from a fresh pseudo-random vector
  int kept       = 0;      // Ritz pairs taken: min(k, m_eff)
  bool converged = false;
  std::vector<double> theta;  // [kept] ascending
  std::vector<double> arrow;  // [kept] beta_last * s[m_eff - 1][i] (zero after a collapse)
  std::vector<double> s;      // [m_eff, kept] row-major: the Ritz vectors are s^T V
};

// alpha [m_end], beta [m_end + 1] (beta[j + 1] = the norm that made basis vector j + 1); steps locked .. m_end - 1 were taken
inline cycle end_of_cycle(int64_t n, int k, int locked, int m_end, const double* theta, const double* arrow, const double* alpha,
                          const double* beta, double tol, double collapse)
{
  cycle c;
  c.m_eff = m_end;
  for (int j = locked; j < m_end; ++j)
    if (!(beta[j + 1] > collapse)) {  // (a NaN counts as collapsed)
      c.m_eff     = j + 1;
      c.collapsed = true;
      break;
    }
  const int m = c.m_eff;
  std::vector<double> t = projected_matrix(m, locked, theta, arrow, alpha, beta), evals, vecs;
  jacobi_eigh(m, t, evals, vecs);
  c.kept = std::min(k, m);
  const double beta_last = c.collapsed ? 0.0 : beta[m];
  c.theta.assign(evals.begin(), evals.begin() + c.kept);
  c.arrow.resize((size_t)c.kept);
  c.s.resize((size_t)m * c.kept);
  double worst = 0.0;
  for (int i = 0; i < c.kept; ++i) {
    c.arrow[(size_t)i] = beta_last * vecs[(size_t)(m - 1) * m + i];
    worst              = std::max(worst, std::fabs(c.arrow[(size_t)i]));
    for (int r = 0; r < m; ++r) c.s[(size_t)r * c.kept + i] = vecs[(size_t)r * m + i];
  }
  c.converged = c.kept == k && (c.collapsed ? (int64_t)m == n : worst <= stop_tolerance(tol));
  return c;
}

}  // namespace spectral_host
}  // namespace cuvs_amd

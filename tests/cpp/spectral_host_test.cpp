// Stand-alone program over cuvs_amd/csrc/spectral_host.hpp: prints arrow-plus-tridiagonal matrices of order 1, 2, 21 and 129 with
// the eigen-decomposition the cyclic Jacobi solver gives them (tests/test_spectral_cpu.py compares with numpy.linalg.eigh), and
// checks the decisions at the end of a cycle on hand-made inputs.
#include "spectral_host.hpp"

#include <cstdio>
#include <cstdlib>

namespace H = cuvs_amd::spectral_host;

#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::printf("FAILED %s (line %d)\n", #cond, __LINE__);              \
      return 1;                                                           \
    }                                                                     \
  } while (0)

static double value(uint32_t salt, uint32_t i) { return (double)H::hashed_uniform(H::seed_fold(7), salt, i); }

int main()
{
  const int orders[4] = {1, 2, 21, 129};
  for (int m : orders) {
    const int locked = m / 3;
    std::vector<double> theta((size_t)m), arrow((size_t)m), alpha((size_t)m), beta((size_t)m + 1);
    for (int i = 0; i < m; ++i) {
      theta[(size_t)i] = 0.01 * i;
      arrow[(size_t)i] = 1e-3 * value(1, (uint32_t)i);
      alpha[(size_t)i] = 1.0 + value(2, (uint32_t)i);
      beta[(size_t)i]  = 0.5 + 0.4 * value(3, (uint32_t)i);
    }
    std::vector<double> t = H::projected_matrix(m, locked, theta.data(), arrow.data(), alpha.data(), beta.data());
    std::printf("order %d\n", m);
    for (double v : t) std::printf("%.17g\n", v);
    std::vector<double> evals, vecs;
    H::jacobi_eigh(m, t, evals, vecs);
    for (double v : evals) std::printf("%.17g\n", v);
    for (double v : vecs) std::printf("%.17g\n", v);
  }

  // the basis size: the reference's rule, raised to k + 1
  CHECK(H::ncv_rule(1000, 4) == 20 && H::ncv_rule(1000, 15) == 31 && H::ncv_rule(22, 4) == 18 && H::ncv_rule(3, 2) == 3);
  CHECK(H::stop_tolerance(0.0) == H::kEps32 && H::stop_tolerance(1e-5) == H::kEps32 && H::stop_tolerance(1e-8) == 1e-8);
  // the start vector is in [-1, 1) and differs between salts
  for (uint32_t i = 0; i < 1000; ++i) {
    const float a = H::hashed_uniform(H::seed_fold(0), 0, i);
    CHECK(a >= -1.0f && a < 1.0f);
  }
  CHECK(H::hashed_uniform(H::seed_fold(0), 0, 5) != H::hashed_uniform(H::seed_fold(0), 1, 5));
  CHECK(H::seed_fold(1) != H::seed_fold(uint64_t(1) << 32));

  {  // a first cycle of 4 steps on diag(1, 2, 3, 4) seen through a tridiagonal with a small last beta: converged
    const double alpha[4] = {1, 2, 3, 4}, beta[5] = {0, 0.1, 0.1, 0.1, 1e-9};
    H::cycle c = H::end_of_cycle(100, 2, 0, 4, nullptr, nullptr, alpha, beta, 0.0, 1e-12);
    CHECK(c.m_eff == 4 && !c.collapsed && c.kept == 2 && c.converged);
    CHECK(c.theta[0] < c.theta[1] && c.theta[0] < 1.0 && c.s.size() == 8);
    // the same with a large last beta: not converged, the arrow is beta_last times the last row of s
    const double beta2[5] = {0, 0.1, 0.1, 0.1, 0.7};
    c = H::end_of_cycle(100, 2, 0, 4, nullptr, nullptr, alpha, beta2, 0.0, 1e-12);
    CHECK(!c.converged && !c.collapsed);
    CHECK(std::fabs(c.arrow[0] - 0.7 * c.s[3 * 2 + 0]) < 1e-15);
    // a collapsed step 2: the projected problem has order 2 and the arrow is zero; not converged unless the basis is all of R^n
    const double beta3[5] = {0, 0.1, 1e-13, 0.1, 0.7};
    c = H::end_of_cycle(100, 2, 0, 4, nullptr, nullptr, alpha, beta3, 0.0, 1e-12);
    CHECK(c.collapsed && c.m_eff == 2 && c.kept == 2 && !c.converged && c.arrow[0] == 0.0 && c.arrow[1] == 0.0);
    c = H::end_of_cycle(2, 1, 0, 2, nullptr, nullptr, alpha, beta3, 0.0, 1e-12);
    CHECK(c.collapsed && c.m_eff == 2 && c.kept == 1 && c.converged);
    // fewer vectors than asked for are never converged
    const double beta4[5] = {0, 1e-13, 0.1, 0.1, 0.7};
    c = H::end_of_cycle(100, 2, 0, 4, nullptr, nullptr, alpha, beta4, 0.0, 1e-12);
    CHECK(c.collapsed && c.m_eff == 1 && c.kept == 1 && !c.converged);
    // a NaN norm counts as collapsed
    const double beta5[5] = {0, 0.1, std::nan(""), 0.1, 0.7};
    c = H::end_of_cycle(100, 2, 0, 4, nullptr, nullptr, alpha, beta5, 0.0, 1e-12);
    CHECK(c.collapsed && c.m_eff == 2);
  }
  std::printf("spectral host OK\n");
  return 0;
}

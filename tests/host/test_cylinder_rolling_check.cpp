// Stand-alone driver of what the cylinders' rolling and twisting setters (docs/SPEC.md §2.21) take from
// csrc/surface_coefficients.hpp, for tests/test_cylinder_rolling_check.py: built plainly and with g++ under
// AddressSanitizer + UBSan.  It runs the argument check of shstep_set_rolling_cyl and shstep_set_twisting_cyl on
// accepted and refused inputs and prints one line per case, "ok" or the message; then the `roll` switch over a cylinder
// record and the [4][n] image of the device table, one line each.  The arrays are heap blocks of exactly the documented
// size, so a read past ncyl entries is a sanitizer report.
#include <cstdio>
#include <limits>
#include <vector>

#include "surface_coefficients.hpp"

using namespace shp;

// the checks as the two setters call them
static std::string check_rolling(int ncyl, int nset, const double* mu_r, const double* gamma_r)
{
  const double* tabs[2] = {mu_r, gamma_r};
  const char* names[2] = {"rolling coefficient mu_r", "rolling coefficient gamma_r"};
  return check_surface_coefficients(kCylinderSurface, "rolling resistance", ncyl, nset, 2, tabs, names, false);
}

static std::string check_twisting(int ncyl, int nset, const double* mu_tw, const double* gamma_tw)
{
  const double* tabs[2] = {mu_tw, gamma_tw};
  const char* names[2] = {"twisting coefficient mu_tw", "twisting coefficient gamma_tw"};
  return check_surface_coefficients(kCylinderSurface, "twisting resistance", ncyl, nset, 2, tabs, names, false);
}

static void show(const char* label, const std::string& m) { std::printf("%s: %s\n", label, m.empty() ? "ok" : m.c_str()); }

static void show_switch(const char* label, const SurfaceCoefficients& r)
{
  const SurfaceSwitches on = derive_surface_switches(r);
  std::printf("%s: roll %d any %d damp %d fric %d hist %d\n", label, (int)on.roll, (int)on.any(), (int)on.damp, (int)on.fric, (int)on.hist);
}

int main()
{
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  for (int n : {1, 8}) {
    std::vector<double> mu((size_t)n, 0.05), g((size_t)n, 3.0);
    mu[0] = 0.0;   // a cylinder without the kind beside seven with it
    show("rolling accepted", check_rolling(n, n, mu.data(), g.data()));
    show("twisting accepted", check_twisting(n, n, mu.data(), g.data()));
  }
  show("none set", check_rolling(0, 0, nullptr, nullptr));
  std::vector<double> mu = {0.0, 0.05, 0.5}, g = {1.0, 2.0, 0.0};
  show("rolling count", check_rolling(3, 2, mu.data(), g.data()));
  show("twisting count before any cylinder", check_twisting(3, 0, mu.data(), g.data()));
  show("rolling null mu", check_rolling(3, 3, nullptr, g.data()));
  show("twisting null gamma", check_twisting(3, 3, mu.data(), nullptr));
  mu[2] = -0.5;
  show("rolling negative mu", check_rolling(3, 3, mu.data(), g.data()));
  show("twisting negative mu", check_twisting(3, 3, mu.data(), g.data()));
  mu[2] = 0.5;
  g[1] = -2.0;
  show("rolling negative gamma", check_rolling(3, 3, mu.data(), g.data()));
  g[1] = nan;
  show("twisting nan gamma", check_twisting(3, 3, mu.data(), g.data()));
  g[1] = 2.0;
  mu[0] = inf;
  show("rolling inf mu", check_rolling(3, 3, mu.data(), g.data()));

  // the switch over a cylinder record: a kind needs both of its coefficients on the same cylinder
  SurfaceCoefficients r;
  r.reset(3);
  show_switch("fresh", r);
  r.mu_r = {0.05, 0.0, 0.0};
  r.gamma_r = {0.0, 3.0, 0.0};
  show_switch("mu_r and gamma_r on different cylinders", r);
  r.gamma_r[0] = 3.0;
  show_switch("rolling on cylinder 0", r);
  r.Omega = {0.7, 0.0, 0.0};
  show_switch("and a rotation", r);
  r.mu_r[0] = 0.0;
  r.mu_tw = {0.0, 0.0, 0.03};
  r.gamma_tw = {0.0, 0.0, 2.0};
  show_switch("twisting alone on cylinder 2", r);
  r.gamma = {0.0, 4.0, 0.0};
  show_switch("and damping", r);
  r.reset(3);
  show_switch("reset", r);

  // the [4][n] image of the device table
  r.mu_r = {1.0, 2.0, 3.0};
  r.gamma_r = {4.0, 5.0, 6.0};
  r.mu_tw = {7.0, 8.0, 9.0};
  r.gamma_tw = {10.0, 11.0, 12.0};
  const std::vector<double> h = pack_surface_tables({&r.mu_r, &r.gamma_r, &r.mu_tw, &r.gamma_tw});
  std::printf("image %zu:", h.size());
  for (double v : h) std::printf(" %g", v);
  std::printf("\n");
  return 0;
}

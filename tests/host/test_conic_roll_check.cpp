// Host-only program for tests/test_conic_roll_check.py: what shstep_set_rolling_con and shstep_set_twisting_con
// (docs/SPEC.md §2.24) accept, through check_conic_resistance of csrc/cone_check.hpp, the words a cone pass without
// twists is told, and what a record with the four coefficients switches on (csrc/surface_coefficients.hpp).  Prints
// "label: message" per case ("ok" for an accepted one).  No HIP, so that it builds with g++ under AddressSanitizer + UBSan.
#include <cstdio>
#include <limits>
#include <string>

#include "cone_check.hpp"

using namespace shp;

static void show(const char* label, const std::string& msg) { std::printf("%s: %s\n", label, msg.empty() ? "ok" : msg.c_str()); }

static std::string switches(const SurfaceCoefficients& r)
{
  const SurfaceSwitches on = derive_surface_switches(r);
  return surface_msg("damp %d fric %d hist %d roll %d any %d", (int)on.damp, (int)on.fric, (int)on.hist, (int)on.roll, (int)on.any());
}

int main()
{
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const double mu[2] = {0.05, 0.0}, ga[2] = {3.0, 0.0}, neg[2] = {1.0, -0.5}, bad[2] = {nan, 1.0}, big[2] = {1.0, inf};
  const double eight[8] = {1, 2, 3, 4, 5, 6, 7, 8};
  const double* ok2[2] = {mu, ga};
  const double* ok8[2] = {eight, eight};
  const double* none[2] = {nullptr, nullptr};
  const double* null1[2] = {mu, nullptr};
  const double* negmu[2] = {neg, ga};
  const double* nangamma[2] = {mu, bad};
  const double* infgamma[2] = {mu, big};
  show("accepted", check_conic_resistance("rolling", 2, 2, ok2));
  show("eight", check_conic_resistance("twisting", 8, 8, ok8));
  show("none", check_conic_resistance("rolling", 0, 0, none));
  show("count", check_conic_resistance("twisting", 3, 2, ok8));
  show("before the cones", check_conic_resistance("rolling", 1, 0, ok2));
  show("null table", check_conic_resistance("rolling", 2, 2, null1));
  show("negative", check_conic_resistance("rolling", 2, 2, negmu));
  show("nan", check_conic_resistance("twisting", 2, 2, nangamma));
  show("inf", check_conic_resistance("rolling", 2, 2, infgamma));
  std::printf("null twist: %s\n", conic_resistance_null_twist());
  // a kind needs both of its coefficients on the same cone; the two setters in either order give the same switches
  SurfaceCoefficients a, b;
  a.reset(2);
  b.reset(2);
  a.mu_r = {0.05, 0.0};
  a.gamma_r = {0.0, 3.0};       // a mu_r without a gamma_r on the same cone
  std::printf("split rolling: %s\n", switches(a).c_str());
  a.gamma_r = {3.0, 0.0};
  std::printf("rolling alone: %s\n", switches(a).c_str());
  b.mu_tw = {0.0, 0.03};
  b.gamma_tw = {0.0, 2.0};
  std::printf("twisting alone: %s\n", switches(b).c_str());
  a.mu_tw = b.mu_tw;
  a.gamma_tw = b.gamma_tw;
  b.mu_r = a.mu_r;
  b.gamma_r = a.gamma_r;
  std::printf("rolling then twisting: %s\n", switches(a).c_str());
  std::printf("twisting then rolling: %s\n", switches(b).c_str());
  a.mu_r = {0.0, 0.0};
  std::printf("rolling to 0: %s\n", switches(a).c_str());
  a.gamma_tw = {0.0, 0.0};
  std::printf("both to 0: %s\n", switches(a).c_str());
  b.reset(2);
  b.Omega = {1.7, 0.0};         // the rotation alone is no coefficient
  std::printf("rotation alone: %s\n", switches(b).c_str());
  b.mu = {0.5, 0.5};
  b.k_t = {4000.0, 0.0};
  b.mu_r = {0.0, 0.05};
  b.gamma_r = {0.0, 3.0};
  std::printf("spring and rolling: %s\n", switches(b).c_str());
  b.reset(2);
  std::printf("reset: %s\n", switches(b).c_str());
  return 0;
}

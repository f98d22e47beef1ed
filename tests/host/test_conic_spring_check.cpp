// Host-only program for tests/test_conic_spring_check.py: what shstep_set_conic_tangential_spring (docs/SPEC.md §2.23)
// accepts, through check_conic_spring of csrc/cone_check.hpp, and what a record with a k_t switches on
// (csrc/surface_coefficients.hpp).  Prints "label: message" per case ("ok" for an accepted one).  No HIP, so that it
// builds with g++ under AddressSanitizer + UBSan.
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
  const double two[2] = {4000.0, 0.0}, neg[2] = {1.0, -2.0}, bad[2] = {nan, 1.0}, big[2] = {1.0, inf};
  const double eight[8] = {1, 2, 3, 4, 5, 6, 7, 8};
  show("accepted", check_conic_spring(2, 2, two));
  show("eight", check_conic_spring(8, 8, eight));
  show("none", check_conic_spring(0, 0, nullptr));
  show("count", check_conic_spring(3, 2, eight));
  show("before the cones", check_conic_spring(2, 0, two));
  show("null table", check_conic_spring(2, 2, nullptr));
  show("negative", check_conic_spring(2, 2, neg));
  show("nan", check_conic_spring(2, 2, bad));
  show("inf", check_conic_spring(2, 2, big));
  // the two setters in either order: the same switches
  SurfaceCoefficients a, b;
  a.reset(2);
  b.reset(2);
  a.k_t.assign(two, two + 2);
  std::printf("spring alone: %s\n", switches(a).c_str());
  a.mu = {0.5, 0.5};           // gamma_t stays 0: history without viscous friction
  b.mu = {0.5, 0.5};
  std::printf("friction alone: %s\n", switches(b).c_str());
  b.k_t.assign(two, two + 2);
  std::printf("spring then mu: %s\n", switches(a).c_str());
  std::printf("mu then spring: %s\n", switches(b).c_str());
  a.mu = {0.0, 0.5};           // the mu of the last history cone to 0: cone 1 has a mu but no k_t
  std::printf("last mu to 0: %s\n", switches(a).c_str());
  b.k_t = {0.0, 0.0};
  std::printf("every k_t to 0: %s\n", switches(b).c_str());
  b.reset(2);
  std::printf("reset: %s\n", switches(b).c_str());
  return 0;
}

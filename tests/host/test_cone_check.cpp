// Host-only program for tests/test_cone_check.py: what shstep_set_cones and the cone coefficient setters (docs/SPEC.md
// §2.22) accept, through csrc/cone_check.hpp and csrc/surface_coefficients.hpp.  Prints "label: message" per case ("ok"
// for an accepted one).  No HIP, so that it builds with g++ under AddressSanitizer + UBSan.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "cone_check.hpp"

using namespace shp;

static void show(const char* label, const std::string& msg) { std::printf("%s: %s\n", label, msg.empty() ? "ok" : msg.c_str()); }

int main()
{
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const double c30 = std::cos(0.5235987755982988), s30 = std::sin(0.5235987755982988);
  const std::vector<double> good = {0.1, 0.2, 0.3, 2.0 / 7.0, 3.0 / 7.0, 6.0 / 7.0, c30, s30};
  const double kn[9] = {1, 1, 1, 1, 1, 1, 1, 1, 1}, ex[9] = {1, 1, 1, 1, 1, 1, 1, 1, 1};
  auto with = [&](int k, double v) { std::vector<double> c = good; c[k] = v; return c; };
  show("accepted", check_cones(1, good.data(), kn, ex));
  show("none", check_cones(0, nullptr, nullptr, nullptr));
  std::vector<double> eight, nine;
  for (int k = 0; k < 9; ++k) nine.insert(nine.end(), good.begin(), good.end());
  eight.assign(nine.begin(), nine.begin() + 64);
  show("eight", check_cones(8, eight.data(), kn, ex));
  show("nine", check_cones(9, nine.data(), kn, ex));
  show("negative count", check_cones(-1, good.data(), kn, ex));
  show("null", check_cones(1, nullptr, kn, ex));
  show("axis length", check_cones(1, with(5, 0.9).data(), kn, ex));
  show("cos < 0", check_cones(1, with(6, -c30).data(), kn, ex));
  show("cos 0", check_cones(1, std::vector<double>{0, 0, 0, 0, 0, 1, 0.0, 1.0}.data(), kn, ex));
  show("sin 0", check_cones(1, std::vector<double>{0, 0, 0, 0, 0, 1, 1.0, 0.0}.data(), kn, ex));
  show("off the circle", check_cones(1, with(7, s30 + 1e-9).data(), kn, ex));
  show("one ulp off", check_cones(1, with(7, std::nextafter(s30, 1.0)).data(), kn, ex));
  show("near pi/2", check_cones(1, std::vector<double>{0, 0, 0, 0, 0, 1, std::cos(1.5707963167948966), std::sin(1.5707963167948966)}.data(), kn, ex));
  show("cos nan", check_cones(1, with(6, nan).data(), kn, ex));
  show("apex inf", check_cones(1, with(0, inf).data(), kn, ex));
  const double knneg[1] = {-1.0}, exlow[1] = {0.5}, knnan[1] = {nan};
  show("kn < 0", check_cones(1, good.data(), knneg, ex));
  show("exponent < 1", check_cones(1, good.data(), kn, exlow));
  show("kn nan", check_cones(1, good.data(), knnan, ex));
  // the coefficient setters' check with the cone's words
  const double g2[2] = {1.0, 0.0}, gneg[2] = {1.0, -2.0}, gnan[2] = {nan, 0.0}, om[2] = {-3.0, 2.0}, oinf[2] = {inf, 0.0};
  const char* dn[1] = {"damping coefficient"};
  const char* rn[1] = {"angular velocity"};
  const double* t = g2;
  show("coefficients accepted", check_surface_coefficients(kConeSurface, "damping", 2, 2, 1, &t, dn, false));
  show("count", check_surface_coefficients(kConeSurface, "damping", 3, 2, 1, &t, dn, false));
  const double* tn = nullptr;
  show("null table", check_surface_coefficients(kConeSurface, "damping", 2, 2, 1, &tn, dn, false));
  t = gneg;
  show("negative", check_surface_coefficients(kConeSurface, "damping", 2, 2, 1, &t, dn, false));
  t = gnan;
  show("nan", check_surface_coefficients(kConeSurface, "damping", 2, 2, 1, &t, dn, false));
  t = om;
  show("negative rotation", check_surface_coefficients(kConeSurface, "rotation", 2, 2, 1, &t, rn, true));
  t = oinf;
  show("inf rotation", check_surface_coefficients(kConeSurface, "rotation", 2, 2, 1, &t, rn, true));
  return 0;
}

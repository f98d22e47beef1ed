// Stand-alone driver of csrc/cylinder_check.hpp and of the cylinders' side of csrc/surface_coefficients.hpp for
// tests/test_cyl_capi.py: built with g++ under AddressSanitizer +
// UBSan, it runs the argument checks of the cylinder setters (docs/SPEC.md §2.18) on accepted and refused inputs and
// prints one line per case: "ok" or the message.  The arrays are heap blocks of exactly the documented size, so a read
// past ncyl entries is a sanitizer report.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "cylinder_check.hpp"
#include "surface_coefficients.hpp"

using shp::check_cylinders;

// the coefficient setters' check as the cylinders call it
static std::string check_cylinder_coefficients(const char* what, int ncyl, int nset, int ntab, const double* const* tabs,
                                               const char* const* names, bool any_sign)
{
  return shp::check_surface_coefficients(shp::kCylinderSurface, what, ncyl, nset, ntab, tabs, names, any_sign);
}

static void show(const char* label, const std::string& m) { std::printf("%s: %s\n", label, m.empty() ? "ok" : m.c_str()); }

int main()
{
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  for (int n : {0, 1, 8}) {
    std::vector<double> c(7 * (size_t)n), kn((size_t)n, 1000.0), ex((size_t)n, 1.25);
    for (int k = 0; k < n; ++k) {
      double* p = &c[7 * (size_t)k];
      p[0] = 0.1 * k; p[1] = -0.2; p[2] = 0.3; p[3] = 2.0 / 7.0; p[4] = 3.0 / 7.0; p[5] = 6.0 / 7.0; p[6] = 1.0 + k;
    }
    show("accepted", check_cylinders(n, n ? c.data() : nullptr, n ? kn.data() : nullptr, n ? ex.data() : nullptr));
  }
  {
    std::vector<double> c(7 * 9, 0.0), kn(9, 1.0), ex(9, 1.0);
    show("nine", check_cylinders(9, c.data(), kn.data(), ex.data()));
    show("negative count", check_cylinders(-1, c.data(), kn.data(), ex.data()));
    show("null", check_cylinders(1, nullptr, kn.data(), ex.data()));
  }
  struct Bad { const char* label; int index; double value; double kn, ex; };
  const Bad bad[] = {{"axis length", 5, 1.0 + 1e-9, 1.0, 1.0}, {"zero axis", -1, 0.0, 1.0, 1.0}, {"radius 0", 6, 0.0, 1.0, 1.0},
                     {"radius < 0", 6, -2.0, 1.0, 1.0}, {"radius nan", 6, nan, 1.0, 1.0}, {"point inf", 0, inf, 1.0, 1.0},
                     {"kn < 0", 6, 2.0, -1.0, 1.0}, {"kn nan", 6, 2.0, nan, 1.0}, {"exponent < 1", 6, 2.0, 1.0, 0.5},
                     {"exponent inf", 6, 2.0, 1.0, inf}};
  for (const Bad& b : bad) {
    std::vector<double> c = {0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 2.0}, kn = {b.kn}, ex = {b.ex};
    if (b.index >= 0) c[(size_t)b.index] = b.value;
    else c[5] = 0.0;
    show(b.label, check_cylinders(1, c.data(), kn.data(), ex.data()));
  }
  const char* names[2] = {"coefficient a", "coefficient b"};
  {
    std::vector<double> a = {0.0, 2.0, 0.5}, b = {1.0, 0.0, 3.0};
    const double* tabs[2] = {a.data(), b.data()};
    show("coefficients accepted", check_cylinder_coefficients("friction", 3, 3, 2, tabs, names, false));
    show("count", check_cylinder_coefficients("friction", 3, 2, 2, tabs, names, false));
    show("none set", check_cylinder_coefficients("friction", 0, 0, 2, tabs, names, false));
    const double* holed[2] = {a.data(), nullptr};
    show("null table", check_cylinder_coefficients("friction", 3, 3, 2, holed, names, false));
    a[2] = -0.5;
    show("negative", check_cylinder_coefficients("friction", 3, 3, 2, tabs, names, false));
    show("negative rotation", check_cylinder_coefficients("rotation", 3, 3, 1, tabs, names, true));
    a[2] = nan;
    show("nan", check_cylinder_coefficients("damping", 3, 3, 1, tabs, names, false));
    a[2] = inf;
    show("inf rotation", check_cylinder_coefficients("rotation", 3, 3, 1, tabs, names, true));
  }
  return 0;
}

// Stand-alone driver of the check of the cylinders' spring setter (csrc/surface_coefficients.hpp) for
// tests/test_cyl_history_capi.py: built with
// g++ under AddressSanitizer + UBSan, it runs the argument check of shstep_set_cyl_tangential_spring (docs/SPEC.md §2.19)
// on accepted and refused inputs and prints one line per case: "ok" or the message.  The arrays are heap blocks of
// exactly the documented size, so a read past ncyl entries is a sanitizer report.
#include <cstdio>
#include <limits>
#include <vector>

#include "surface_coefficients.hpp"

// the check as shstep_set_cyl_tangential_spring calls it
static std::string check_cylinder_spring(int ncyl, int nset, const double* kt)
{
  const char* names[1] = {"tangential spring k_t"};
  return shp::check_surface_coefficients(shp::kCylinderSurface, "tangential spring", ncyl, nset, 1, &kt, names, false);
}

static void show(const char* label, const std::string& m) { std::printf("%s: %s\n", label, m.empty() ? "ok" : m.c_str()); }

int main()
{
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  for (int n : {1, 8}) {
    std::vector<double> kt((size_t)n, 4000.0);
    kt[0] = 0.0;   // a cylinder without a spring beside seven with one
    show("accepted", check_cylinder_spring(n, n, kt.data()));
  }
  show("none set", check_cylinder_spring(0, 0, nullptr));
  std::vector<double> kt = {0.0, 2.0, 0.5};
  show("count", check_cylinder_spring(3, 2, kt.data()));
  show("count before any cylinder", check_cylinder_spring(3, 0, kt.data()));
  show("null", check_cylinder_spring(3, 3, nullptr));
  kt[2] = -0.5;
  show("negative", check_cylinder_spring(3, 3, kt.data()));
  kt[2] = nan;
  show("nan", check_cylinder_spring(3, 3, kt.data()));
  kt[2] = inf;
  show("inf", check_cylinder_spring(3, 3, kt.data()));
  return 0;
}

// cylinder_check.hpp — what the cylinder setters of include/shstep.h (docs/SPEC.md §2.18) accept: the argument checks of
// shstep_set_cylinders, of the three coefficient setters and of the spring setter of §2.19, as plain host functions that
// return the message of the first fault ("" for none).  No HIP call and no context in here, so that
// tests/host/test_cylinder_check.cpp and test_cylinder_spring_check.cpp can build them under AddressSanitizer + UBSan;
// shstep_cylinders.hip is the only other includer.
#pragma once
#include <cmath>
#include <cstdio>
#include <string>

namespace shp {

constexpr int kCylinderLimit = 8;   // SHSTEP_MAX_CYLINDERS

template <typename... A>
inline std::string cyl_msg(const char* fmt, A... a)
{
  char buf[256];
  std::snprintf(buf, sizeof buf, fmt, a...);
  return buf;
}

// cyl7[7c..] = a[3], axis[3], Rc; kn[c], exponent[c]
inline std::string check_cylinders(int ncyl, const double* cyl7, const double* kn, const double* exponent)
{
  if (ncyl < 0 || ncyl > kCylinderLimit) return cyl_msg("cylinders: %d cylinders, 0..%d are accepted", ncyl, kCylinderLimit);
  if (ncyl > 0 && (!cyl7 || !kn || !exponent)) return "cylinders: null array pointer";
  for (int c = 0; c < ncyl; ++c) {
    const double* p = cyl7 + 7 * c;
    for (int k = 0; k < 7; ++k)
      if (!std::isfinite(p[k])) return cyl_msg("cylinder %d: a number that is not finite", c);
    if (!std::isfinite(kn[c]) || !std::isfinite(exponent[c])) return cyl_msg("cylinder %d: a number that is not finite", c);
    const double nn = std::sqrt(p[3] * p[3] + p[4] * p[4] + p[5] * p[5]);
    if (!(std::fabs(nn - 1.0) <= 1e-12)) return cyl_msg("cylinder %d: the axis has length %.17g, not 1", c, nn);
    if (!(p[6] > 0.0)) return cyl_msg("cylinder %d: radius %g must be > 0", c, p[6]);
    if (kn[c] < 0.0) return cyl_msg("cylinder %d: kn %g < 0", c, kn[c]);
    if (exponent[c] < 1.0) return cyl_msg("cylinder %d: exponent %g < 1", c, exponent[c]);
  }
  return "";
}

// The coefficient setters' common part: the count against the cylinders set, null pointers, every value finite and,
// unless `any_sign` (the rotation), >= 0.
inline std::string check_cylinder_coefficients(const char* what, int ncyl, int nset, int ntab, const double* const* tabs,
                                               const char* const* names, bool any_sign)
{
  if (ncyl != nset) return cyl_msg("cylinder %s: %d coefficients for %d cylinders (call it after shstep_set_cylinders)", what, ncyl, nset);
  if (ncyl == 0) return "";
  for (int k = 0; k < ntab; ++k)
    if (!tabs[k]) return cyl_msg("cylinder %s: null array pointer", what);
  for (int c = 0; c < ncyl; ++c)
    for (int k = 0; k < ntab; ++k) {
      const double v = tabs[k][c];
      if (!std::isfinite(v)) return cyl_msg("cylinder %d: %s %g must be finite", c, names[k], v);
      if (!any_sign && !(v >= 0.0)) return cyl_msg("cylinder %d: %s %g must be finite and >= 0", c, names[k], v);
    }
  return "";
}

// shstep_set_cyl_tangential_spring (SPEC §2.19): one k_t,c per cylinder set, finite and >= 0.
inline std::string check_cylinder_spring(int ncyl, int nset, const double* kt)
{
  const char* names[1] = {"tangential spring k_t"};
  return check_cylinder_coefficients("tangential spring", ncyl, nset, 1, &kt, names, false);
}

}  // namespace shp

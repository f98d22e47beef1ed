// cylinder_check.hpp — what shstep_set_cylinders of include/shstep.h (docs/SPEC.md §2.18) accepts: its argument check as
// a plain host function that returns the message of the first fault ("" for none).  The coefficient setters' check is
// surface_coefficients.hpp's, shared with the planar walls.  No HIP call and no context in here, so that
// tests/host/test_cylinder_check.cpp can build it under AddressSanitizer + UBSan; shstep_cylinders.hip is the only other
// includer.
#pragma once
#include <cmath>
#include <string>

#include "surface_coefficients.hpp"   // surface_msg

namespace shp {

constexpr int kCylinderLimit = 8;   // SHSTEP_MAX_CYLINDERS

// cyl7[7c..] = a[3], axis[3], Rc; kn[c], exponent[c]
inline std::string check_cylinders(int ncyl, const double* cyl7, const double* kn, const double* exponent)
{
  if (ncyl < 0 || ncyl > kCylinderLimit) return surface_msg("cylinders: %d cylinders, 0..%d are accepted", ncyl, kCylinderLimit);
  if (ncyl > 0 && (!cyl7 || !kn || !exponent)) return "cylinders: null array pointer";
  for (int c = 0; c < ncyl; ++c) {
    const double* p = cyl7 + 7 * c;
    for (int k = 0; k < 7; ++k)
      if (!std::isfinite(p[k])) return surface_msg("cylinder %d: a number that is not finite", c);
    if (!std::isfinite(kn[c]) || !std::isfinite(exponent[c])) return surface_msg("cylinder %d: a number that is not finite", c);
    const double nn = std::sqrt(p[3] * p[3] + p[4] * p[4] + p[5] * p[5]);
    if (!(std::fabs(nn - 1.0) <= 1e-12)) return surface_msg("cylinder %d: the axis has length %.17g, not 1", c, nn);
    if (!(p[6] > 0.0)) return surface_msg("cylinder %d: radius %g must be > 0", c, p[6]);
    if (kn[c] < 0.0) return surface_msg("cylinder %d: kn %g < 0", c, kn[c]);
    if (exponent[c] < 1.0) return surface_msg("cylinder %d: exponent %g < 1", c, exponent[c]);
  }
  return "";
}

}  // namespace shp

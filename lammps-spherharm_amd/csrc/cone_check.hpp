// cone_check.hpp — what shstep_set_cones of include/shstep.h (docs/SPEC.md §2.22) accepts: its argument check as a plain
// host function that returns the message of the first fault ("" for none).  The coefficient setters' check is
// surface_coefficients.hpp's, shared with the planar walls and the cylinders (kConeSurface has the words); the one of the
// tangential spring of §2.23 is check_conic_spring below, on top of it, and so are the one of the rolling and twisting
// resistance of §2.24, check_conic_resistance, and the words of that law's null-twist refusal.  No HIP call
// and no context in here, so that tests/host/test_cone_check.cpp can build it under AddressSanitizer + UBSan;
// shstep_cones.hip is the only other includer.
#pragma once
#include <cfloat>
#include <cmath>
#include <string>

#include "surface_coefficients.hpp"   // surface_msg

namespace shp {

constexpr int kConeLimit = 8;   // SHSTEP_MAX_CONES

// cone8[8k..] = a[3] (the apex), axis[3] (unit, from the apex into the opening), cos theta, sin theta; kn[k], exponent[k].
// The half-angle comes as its cosine and sine, computed once by the caller: both > 0 (0 < theta < pi/2) and
// |cos^2 + sin^2 - 1| <= 4 ulp of 1.
inline std::string check_cones(int ncone, const double* cone8, const double* kn, const double* exponent)
{
  if (ncone < 0 || ncone > kConeLimit) return surface_msg("cones: %d cones, 0..%d are accepted", ncone, kConeLimit);
  if (ncone > 0 && (!cone8 || !kn || !exponent)) return "cones: null array pointer";
  for (int c = 0; c < ncone; ++c) {
    const double* p = cone8 + 8 * c;
    for (int k = 0; k < 8; ++k)
      if (!std::isfinite(p[k])) return surface_msg("cone %d: a number that is not finite", c);
    if (!std::isfinite(kn[c]) || !std::isfinite(exponent[c])) return surface_msg("cone %d: a number that is not finite", c);
    const double nn = std::sqrt(p[3] * p[3] + p[4] * p[4] + p[5] * p[5]);
    if (!(std::fabs(nn - 1.0) <= 1e-12)) return surface_msg("cone %d: the axis has length %.17g, not 1", c, nn);
    if (!(p[6] > 0.0) || !(p[7] > 0.0))
      return surface_msg("cone %d: cos theta %g and sin theta %g must both be > 0 (0 < theta < pi/2)", c, p[6], p[7]);
    const double one = p[6] * p[6] + p[7] * p[7];
    if (!(std::fabs(one - 1.0) <= 4.0 * DBL_EPSILON))
      return surface_msg("cone %d: cos^2 theta + sin^2 theta is %.17g, not 1 within 4 ulp", c, one);
    if (kn[c] < 0.0) return surface_msg("cone %d: kn %g < 0", c, kn[c]);
    if (exponent[c] < 1.0) return surface_msg("cone %d: exponent %g < 1", c, exponent[c]);
  }
  return "";
}

// What shstep_set_conic_tangential_spring (docs/SPEC.md §2.23) accepts: one k_t,k per cone set, each finite and >= 0.
inline std::string check_conic_spring(int ncone, int nset, const double* kt)
{
  return check_surface_setter(kConeSurface, kSetSpring, ncone, nset, &kt);
}

// What shstep_set_rolling_con and shstep_set_twisting_con (docs/SPEC.md §2.24) accept: kind is "rolling" or "twisting",
// tabs the kind's (mu, gamma), one of each per cone set, each finite and >= 0.
inline std::string check_conic_resistance(const char* kind, int ncone, int nset, const double* const* tabs)
{
  return check_surface_setter(kConeSurface, kind[0] == 'r' ? kSetRolling : kSetTwisting, ncone, nset, tabs);
}

// ... and what a cone pass without twists is told while a cone has either kind
inline const char* conic_resistance_null_twist() { return "cone rolling or twisting resistance: null twist pointer"; }

}  // namespace shp

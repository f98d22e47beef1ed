// surface_coefficients.hpp — the coefficients of a surface family, planar walls (docs/SPEC.md §2.10, §2.11, §2.15, §2.17),
// cylinders (§2.18, §2.19, §2.21) or cones (§2.22, §2.23, §2.24), on the host: the argument check of the coefficient
// setters, the record of the tables as the setters took them, the switches derived from a record, and the [k][n] image of
// chosen tables that a device table holds.  The rules exist here once.  Who installs a record (refuse, upload, commit):
// shstep_walls.hip for the walls, install_shell_coefficients of shell_host.hpp for the cylinders and the cones.
// No HIP call and no context in here, so that tests/host/test_surface_coefficients.cpp (and the cylinder-check and
// cone-check programs) can build it under AddressSanitizer + UBSan; shstep_state.hpp (for the types), cylinder_check.hpp
// and cone_check.hpp (for surface_msg and the setters' words), shstep_walls.hip and shell_host.hpp are the only other
// includers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <vector>

namespace shp {

// The words a family's messages are made of.  The walls word a non-finite value their own way, and both wordings stay.
struct SurfaceKind {
  const char* noun;         // "wall"
  const char* plural;       // "walls"
  const char* setter;       // the geometry setter, for the "call it after ..." hint
  const char* not_finite;   // what a non-finite value of a coefficient that must be >= 0 is told
};
constexpr SurfaceKind kWallSurface{"wall", "walls", "shstep_set_walls", "must be finite and >= 0"};
constexpr SurfaceKind kCylinderSurface{"cylinder", "cylinders", "shstep_set_cylinders", "must be finite"};
constexpr SurfaceKind kConeSurface{"cone", "cones", "shstep_set_cones", "must be finite"};   // SPEC §2.22

template <typename... A>
inline std::string surface_msg(const char* fmt, A... a)
{
  char buf[256];
  std::snprintf(buf, sizeof buf, fmt, a...);
  return buf;
}

// The coefficient setters' common part: the count against the surfaces set, null pointers, every value finite and, unless
// `any_sign` (the rotation), >= 0.  The message of the first fault (SHPAIR_EINVAL), "" for none.
inline std::string check_surface_coefficients(const SurfaceKind& kind, const char* what, int n, int nset, int ntab,
                                              const double* const* tabs, const char* const* names, bool any_sign)
{
  if (n != nset)
    return surface_msg("%s %s: %d coefficients for %d %s (call it after %s)", kind.noun, what, n, nset, kind.plural, kind.setter);
  if (n == 0) return "";
  for (int k = 0; k < ntab; ++k)
    if (!tabs[k]) return surface_msg("%s %s: null array pointer", kind.noun, what);
  for (int s = 0; s < n; ++s)
    for (int k = 0; k < ntab; ++k) {
      const double v = tabs[k][s];
      if (!std::isfinite(v)) return surface_msg("%s %d: %s %g %s", kind.noun, s, names[k], v, any_sign ? "must be finite" : kind.not_finite);
      if (!any_sign && !(v >= 0.0)) return surface_msg("%s %d: %s %g must be finite and >= 0", kind.noun, s, names[k], v);
    }
  return "";
}

// The coefficients of n surfaces as the setters took them, [n] each.  A family leaves the tables it has no setter for at 0.
struct SurfaceCoefficients {
  int n = 0;
  std::vector<double> gamma, mu, gamma_t, k_t;          // damping, friction, tangential spring: walls, cylinders, cones
  std::vector<double> mu_r, gamma_r, mu_tw, gamma_tw;   // rolling and twisting resistance: walls, cylinders, cones
  std::vector<double> Omega;                            // angular velocity about the axis: cylinders, cones
  void reset(int n_)   // n_ surfaces, every coefficient 0
  {
    n = n_ > 0 ? n_ : 0;
    for (std::vector<double>* t : {&gamma, &mu, &gamma_t, &k_t, &mu_r, &gamma_r, &mu_tw, &gamma_tw, &Omega}) t->assign((size_t)n, 0.0);
  }
};

// A coefficient setter of the two axial families by its words: what the call is named in a message, its tables in the
// order the caller passes them, each with its name in a message and its place in the record, and whether a value may be
// negative (the rotation).  The cylinders' and the cones' setters are the same seven.
struct SurfaceSetter {
  const char* what;
  int ntab;
  const char* names[2];
  std::vector<double> SurfaceCoefficients::*tabs[2];
  bool any_sign;
};
constexpr SurfaceSetter kSetDamping{"damping", 1, {"damping coefficient", nullptr}, {&SurfaceCoefficients::gamma, nullptr}, false};
constexpr SurfaceSetter kSetFriction{"friction", 2, {"friction coefficient mu", "friction coefficient gamma_t"},
                                        {&SurfaceCoefficients::mu, &SurfaceCoefficients::gamma_t}, false};
constexpr SurfaceSetter kSetRotation{"rotation", 1, {"angular velocity", nullptr}, {&SurfaceCoefficients::Omega, nullptr}, true};
constexpr SurfaceSetter kSetSpring{"tangential spring", 1, {"tangential spring k_t", nullptr}, {&SurfaceCoefficients::k_t, nullptr}, false};
constexpr SurfaceSetter kSetRolling{"rolling resistance", 2, {"rolling coefficient mu_r", "rolling coefficient gamma_r"},
                                       {&SurfaceCoefficients::mu_r, &SurfaceCoefficients::gamma_r}, false};
constexpr SurfaceSetter kSetTwisting{"twisting resistance", 2, {"twisting coefficient mu_tw", "twisting coefficient gamma_tw"},
                                        {&SurfaceCoefficients::mu_tw, &SurfaceCoefficients::gamma_tw}, false};

inline std::string check_surface_setter(const SurfaceKind& kind, const SurfaceSetter& t, int n, int nset, const double* const* tabs)
{
  return check_surface_coefficients(kind, t.what, n, nset, t.ntab, tabs, t.names, t.any_sign);
}

// What a record switches on: the kernel instance of the pass and what the run loops hand it.
struct SurfaceSwitches {
  bool damp = false;   // some gamma != 0
  bool fric = false;   // some surface has mu != 0 and gamma_t != 0
  bool hist = false;   // some surface has mu != 0 and k_t != 0, whichever setter came first: the pass takes a time step
  bool roll = false;   // some surface has a rolling kind (mu_r and gamma_r non-zero) or a twisting kind (mu_tw and gamma_tw)
  bool any() const { return damp || fric || hist || roll; }   // a coefficient is set: the pass reads twists
};

// Omega alone is no coefficient: it enters through the tangential laws only.
inline SurfaceSwitches derive_surface_switches(const SurfaceCoefficients& r)
{
  SurfaceSwitches on;
  for (size_t s = 0; s < (size_t)r.n; ++s) {
    on.damp = on.damp || r.gamma[s] != 0.0;
    on.fric = on.fric || (r.mu[s] != 0.0 && r.gamma_t[s] != 0.0);
    on.hist = on.hist || (r.mu[s] != 0.0 && r.k_t[s] != 0.0);
    on.roll = on.roll || (r.mu_r[s] != 0.0 && r.gamma_r[s] != 0.0) || (r.mu_tw[s] != 0.0 && r.gamma_tw[s] != 0.0);
  }
  return on;
}

// The image a device table of k tables holds: [k][n], the tables of a record one after the other.
inline std::vector<double> pack_surface_tables(std::initializer_list<const std::vector<double>*> tabs)
{
  std::vector<double> h;
  for (const std::vector<double>* t : tabs) h.insert(h.end(), t->begin(), t->end());
  return h;
}

}  // namespace shp

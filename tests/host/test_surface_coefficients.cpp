// Stand-alone host program for csrc/surface_coefficients.hpp: the argument check of the coefficient setters with every
// message as a whole string for both families' words, the record of the coefficients, the switches derived from it (the
// truth table of damp / fric / hist / roll, as the planar walls and the cylinders use it) and the [k][n] image of chosen
// tables.  No HIP.  The arrays are heap blocks of exactly n entries, so a read past them is a sanitizer report.  Prints
// "ok" and returns 0, or every failed check and 1.  tests/test_surface_coefficients.py builds it plainly and with
// -fsanitize=address,undefined.
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "surface_coefficients.hpp"

using namespace shp;

static int fails = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++fails;                                                   \
    }                                                            \
  } while (0)

static void same(int line, const std::string& got, const std::string& want)
{
  if (got == want) return;
  std::printf("FAILED %s:%d: \"%s\", expected \"%s\"\n", __FILE__, line, got.c_str(), want.c_str());
  ++fails;
}
#define SAME(got, want) same(__LINE__, got, want)

static bool equal(const SurfaceSwitches& a, bool damp, bool fric, bool hist, bool roll)
{
  return a.damp == damp && a.fric == fric && a.hist == hist && a.roll == roll && a.any() == (damp || fric || hist || roll);
}

// ---- the check: `geo` is the geometry setter the hint names, `nf` what a non-finite value that must be >= 0 is told
static void check_messages(const SurfaceKind& kind, const std::string& noun, const std::string& plural, const std::string& geo,
                           const std::string& nf)
{
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const char* names[2] = {"friction coefficient mu", "friction coefficient gamma_t"};
  const char* rot[1] = {"angular velocity"};
  std::vector<double> a = {0.0, 2.0, 0.5}, b = {1.0, 0.0, 3.0};
  const double* tabs[2] = {a.data(), b.data()};
  SAME(check_surface_coefficients(kind, "friction", 3, 3, 2, tabs, names, false), "");
  SAME(check_surface_coefficients(kind, "friction", 0, 0, 2, tabs, names, false), "");
  const double* none[2] = {nullptr, nullptr};
  SAME(check_surface_coefficients(kind, "friction", 0, 0, 2, none, names, false), "");   // none set: the pointers are not looked at
  SAME(check_surface_coefficients(kind, "friction", 3, 2, 2, tabs, names, false),
       noun + " friction: 3 coefficients for 2 " + plural + " (call it after " + geo + ")");
  SAME(check_surface_coefficients(kind, "tangential spring", 3, 0, 1, tabs, names, false),
       noun + " tangential spring: 3 coefficients for 0 " + plural + " (call it after " + geo + ")");
  const double* holed[2] = {a.data(), nullptr};
  SAME(check_surface_coefficients(kind, "friction", 3, 3, 2, holed, names, false), noun + " friction: null array pointer");
  SAME(check_surface_coefficients(kind, "friction", 3, 3, 1, holed, names, false), "");   // (only ntab tables are looked at)
  a[2] = -0.5;
  SAME(check_surface_coefficients(kind, "friction", 3, 3, 2, tabs, names, false),
       noun + " 2: friction coefficient mu -0.5 must be finite and >= 0");
  a[2] = 0.5;
  b[1] = -3.0;   // the first fault in surface order, the tables of one surface in their order
  SAME(check_surface_coefficients(kind, "friction", 3, 3, 2, tabs, names, false),
       noun + " 1: friction coefficient gamma_t -3 must be finite and >= 0");
  b[1] = 0.0;
  a[1] = nan;
  SAME(check_surface_coefficients(kind, "friction", 3, 3, 2, tabs, names, false), noun + " 1: friction coefficient mu nan " + nf);
  a[1] = inf;
  SAME(check_surface_coefficients(kind, "friction", 3, 3, 2, tabs, names, false), noun + " 1: friction coefficient mu inf " + nf);
  a[1] = -inf;
  SAME(check_surface_coefficients(kind, "friction", 3, 3, 2, tabs, names, false), noun + " 1: friction coefficient mu -inf " + nf);
  // the rotation: any sign, but finite
  a[1] = -2.5;
  SAME(check_surface_coefficients(kind, "rotation", 3, 3, 1, tabs, rot, true), "");
  a[1] = -inf;
  SAME(check_surface_coefficients(kind, "rotation", 3, 3, 1, tabs, rot, true), noun + " 1: angular velocity -inf must be finite");
  a[1] = nan;
  SAME(check_surface_coefficients(kind, "rotation", 3, 3, 1, tabs, rot, true), noun + " 1: angular velocity nan must be finite");
  SAME(check_surface_coefficients(kind, "rotation", 3, 1, 1, tabs, rot, true),
       noun + " rotation: 3 coefficients for 1 " + plural + " (call it after " + geo + ")");
}

// ---- the record and the switches; `walls`: the family has the rolling tables, else Omega
static void check_switches(bool walls)
{
  SurfaceCoefficients r;
  CHECK(r.n == 0 && equal(derive_surface_switches(r), false, false, false, false));   // before any geometry setter
  r.reset(3);
  CHECK(r.n == 3);
  for (const std::vector<double>* t : {&r.gamma, &r.mu, &r.gamma_t, &r.k_t, &r.mu_r, &r.gamma_r, &r.mu_tw, &r.gamma_tw, &r.Omega}) {
    CHECK(t->size() == 3);
    for (double v : *t) CHECK(v == 0.0);
  }
  CHECK(equal(derive_surface_switches(r), false, false, false, false));
  // damped iff some gamma != 0
  r.gamma = {0.0, 0.0, 2.0};
  CHECK(equal(derive_surface_switches(r), true, false, false, false));
  r.gamma = {0.0, 0.0, 0.0};
  // a mu without a gamma_t on the same surface is no friction, nor is a mu on one surface with a gamma_t on another
  r.mu = {0.5, 0.0, 0.0};
  CHECK(equal(derive_surface_switches(r), false, false, false, false));
  r.gamma_t = {0.0, 2.0, 2.0};
  CHECK(equal(derive_surface_switches(r), false, false, false, false));
  r.gamma_t = {1.0, 0.0, 0.0};
  CHECK(equal(derive_surface_switches(r), false, true, false, false));
  // a mu plus a k_t on the same surface is history with gamma_t == 0; a k_t on another surface is not
  r.gamma_t = {0.0, 0.0, 0.0};
  r.k_t = {0.0, 4000.0, 4000.0};
  CHECK(equal(derive_surface_switches(r), false, false, false, false));
  r.k_t = {4000.0, 0.0, 0.0};
  CHECK(equal(derive_surface_switches(r), false, false, true, false));
  // friction and spring in either order give equal switches (and equal records)
  {
    SurfaceCoefficients p, q;
    p.reset(2);
    q.reset(2);
    p.mu = {0.0, 0.5}; p.gamma_t = {0.0, 2.0};
    const SurfaceSwitches mid_p = derive_surface_switches(p);
    p.k_t = {3.0, 4.0};
    q.k_t = {3.0, 4.0};
    const SurfaceSwitches mid_q = derive_surface_switches(q);
    q.mu = {0.0, 0.5}; q.gamma_t = {0.0, 2.0};
    CHECK(equal(mid_p, false, true, false, false) && equal(mid_q, false, false, false, false));
    CHECK(equal(derive_surface_switches(p), false, true, true, false) && equal(derive_surface_switches(q), false, true, true, false));
    CHECK(p.mu == q.mu && p.gamma_t == q.gamma_t && p.k_t == q.k_t);
    // zeroing the last mu or the last k_t drops hist
    p.mu = {0.0, 0.0};
    CHECK(equal(derive_surface_switches(p), false, false, false, false));
    q.k_t = {3.0, 0.0};
    CHECK(equal(derive_surface_switches(q), false, true, false, false));
    q.k_t = {3.0, 4.0};
    q.gamma = {1.0, 0.0};
    CHECK(equal(derive_surface_switches(q), true, true, true, false));
  }
  if (walls) {
    // a rolling kind needs both of its coefficients on the same wall, and either kind alone sets roll
    r.reset(3);
    r.mu_r = {0.01, 0.0, 0.0};
    CHECK(equal(derive_surface_switches(r), false, false, false, false));
    r.gamma_r = {0.0, 0.5, 0.5};
    CHECK(equal(derive_surface_switches(r), false, false, false, false));
    r.mu_tw = {0.0, 0.0, 0.02};   // a coefficient of each kind on one wall is no kind
    r.gamma_r = {0.0, 0.0, 0.5};
    CHECK(equal(derive_surface_switches(r), false, false, false, false));
    r.gamma_r = {0.5, 0.0, 0.0};
    CHECK(equal(derive_surface_switches(r), false, false, false, true));   // rolling alone
    r.mu_r = {0.0, 0.0, 0.0};
    r.gamma_tw = {0.3, 0.3, 0.0};
    CHECK(equal(derive_surface_switches(r), false, false, false, false));
    r.gamma_tw = {0.0, 0.0, 0.3};
    CHECK(equal(derive_surface_switches(r), false, false, false, true));   // twisting alone
    r.mu_r = {0.01, 0.0, 0.0};
    CHECK(equal(derive_surface_switches(r), false, false, false, true));   // both
  } else {
    // Omega alone sets nothing, and changes nothing beside a coefficient
    r.reset(3);
    r.Omega = {0.5, -2.0, 0.0};
    CHECK(equal(derive_surface_switches(r), false, false, false, false));
    r.mu = {0.0, 0.5, 0.0};
    r.gamma_t = {0.0, 2.0, 0.0};
    CHECK(equal(derive_surface_switches(r), false, true, false, false));
  }
  // the reset clears all, at the new count
  r.gamma = {1.0, 1.0, 1.0};
  r.mu = {1.0, 1.0, 1.0};
  r.gamma_t = r.k_t = r.mu_r = r.gamma_r = r.mu_tw = r.gamma_tw = r.Omega = r.mu;
  CHECK(equal(derive_surface_switches(r), true, true, true, true));
  r.reset(5);
  CHECK(r.n == 5 && r.k_t.size() == 5 && r.Omega.size() == 5 && equal(derive_surface_switches(r), false, false, false, false));
  r.reset(0);
  CHECK(r.n == 0 && r.gamma.empty() && r.mu_tw.empty() && equal(derive_surface_switches(r), false, false, false, false));
}

// ---- the packed images: table k of a [k][n] image starts at k n
static void check_images()
{
  SurfaceCoefficients r;
  r.reset(3);
  r.gamma = {1.0, 2.0, 3.0};
  r.mu = {4.0, 5.0, 6.0};
  r.gamma_t = {7.0, 8.0, 9.0};
  r.Omega = {-1.0, -2.0, -3.0};
  r.mu_r = {10.0, 11.0, 12.0}; r.gamma_r = {13.0, 14.0, 15.0}; r.mu_tw = {16.0, 17.0, 18.0}; r.gamma_tw = {19.0, 20.0, 21.0};
  CHECK(pack_surface_tables({&r.k_t}) == std::vector<double>({0.0, 0.0, 0.0}));
  CHECK(pack_surface_tables({&r.mu, &r.gamma_t}) == std::vector<double>({4.0, 5.0, 6.0, 7.0, 8.0, 9.0}));   // d_wfric
  CHECK(pack_surface_tables({&r.gamma, &r.mu, &r.gamma_t, &r.Omega}) ==
        std::vector<double>({1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, -1.0, -2.0, -3.0}));              // d_ccoef
  const std::vector<double> roll = pack_surface_tables({&r.mu_r, &r.gamma_r, &r.mu_tw, &r.gamma_tw});      // d_wroll
  CHECK(roll.size() == 12);
  for (size_t k = 0; k < roll.size(); ++k) CHECK(roll[k] == 10.0 + (double)k);
  r.reset(0);
  CHECK(pack_surface_tables({&r.mu, &r.gamma_t}).empty());
}

int main()
{
  check_messages(kWallSurface, "wall", "walls", "shstep_set_walls", "must be finite and >= 0");
  check_messages(kCylinderSurface, "cylinder", "cylinders", "shstep_set_cylinders", "must be finite");
  check_switches(true);
  check_switches(false);
  check_images();
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}

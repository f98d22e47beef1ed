// shpair_tables.cpp — shapes, coefficients and the device tables built from them (include/shpair.h): the setters, the
// stateless shape helpers, and shpair_prepare_tables, the one place that refreshes a stale table.  Host code only:
// the tables come from sh_tables.cpp and go up with blocking copies.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/shpair.h"
#include "shpair_ctx.hpp"
#include "sh_const.hpp"
#include "sh_tables.hpp"

using namespace shp;

// a host table into its device buffer (blocking)
template <typename T>
static hipError_t upload_table(DevBuf<T>& b, const std::vector<T>& v)
{
  const hipError_t e = b.ensure(v.size());
  return e != hipSuccess ? e : hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

// every shape and every pair of types has been set; the largest order
static int check_tables_complete(shpair_ctx* c, int* lmax)
{
  if (c->nshapes <= 0 || c->ntypes <= 0) CTX_FAIL(c, SHPAIR_ESTATE, "shpair_set_ntypes() not called");
  int L = -1;
  for (int s = 0; s < c->nshapes; ++s) {
    if (c->shapes[s].lmax < 0) CTX_FAIL(c, SHPAIR_ESTATE, "shape %d was never set", s);
    if (c->shapes[s].lmax > L) L = c->shapes[s].lmax;
  }
  c->any_nonunit_exponent = false;
  for (int a = 1; a <= c->ntypes; ++a)
    for (int b = 1; b <= c->ntypes; ++b) {
      const double k = c->kn[(size_t)a * (c->ntypes + 1) + b], m = c->expo[(size_t)a * (c->ntypes + 1) + b];
      if (std::isnan(k) || std::isnan(m)) CTX_FAIL(c, SHPAIR_ESTATE, "pair_coeff for types %d %d was never set", a, b);
      if (m != 1.0) c->any_nonunit_exponent = true;
    }
  *lmax = L;
  return SHPAIR_OK;
}

static int upload_tables(shpair_ctx* c)
{
  int L = -1;
  RC(check_tables_complete(c, &L));
  std::vector<double> rc_n, rc, scale, cw_n, cw, all, allm, wm, rmax;
  build_recurrence(L, rc_n, scale);
  to_m_major(L, 1, rc_n, rc);
  // cap-frame evaluation of particle i: real-basis coefficients, X matrices, ring scale
  std::vector<double> creal_all, cr, xval, gs;
  std::vector<int> xcol, xinfo;
  for (int s = 0; s < c->nshapes; ++s) {
    const Shape& sh = c->shapes[s];
    build_coefficients(L, sh.lmax, sh.anm.data(), rc_n, scale, cw_n);
    to_m_major(L, 2, cw_n, cw);
    cw.resize(sh_chunk_stride(L), 0.0);
    all.insert(all.end(), cw.begin(), cw.end());
    build_monomial(L, sh.lmax, sh.anm.data(), wm);
    wm.resize(sh_chunk_stride(L), 0.0);
    allm.insert(allm.end(), wm.begin(), wm.end());
    rmax.push_back(sh.rmax);
    real_coefficients(L, sh.lmax, sh.anm.data(), cr);
    creal_all.insert(creal_all.end(), cr.begin(), cr.end());
  }
  build_xmats_ell(L, xval, xcol, xinfo);
  if (xval.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "internal: X matrix row wider than lmax/2+1");
  build_ring_scale(L, gs);
  std::vector<double> jval;
  std::vector<int> jcol;
  build_jpoly_ell(L, jval, jcol);
  if (jval.empty()) CTX_FAIL(c, SHPAIR_EINVAL, "internal: per-azimuth polynomial row wider than lmax/2+1");
  // a kernel still in flight on ANY stream (the caller's, not only the context's) may be reading the old tables
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, upload_table(c->d_creal, creal_all));
  HIPCHK(c, upload_table(c->d_xval, xval));
  HIPCHK(c, upload_table(c->d_xcol, xcol));
  HIPCHK(c, upload_table(c->d_xinfo, xinfo));
  HIPCHK(c, upload_table(c->d_gscale, gs));
  HIPCHK(c, upload_table(c->d_jval, jval));
  HIPCHK(c, upload_table(c->d_jcol, jcol));
  HIPCHK(c, upload_table(c->d_rc, rc));
  HIPCHK(c, upload_table(c->d_coef, all));
  HIPCHK(c, upload_table(c->d_coefm, allm));
  HIPCHK(c, upload_table(c->d_rmax, rmax));
  HIPCHK(c, upload_table(c->d_kn, c->kn));   // unset entries were rejected above; upload as is
  HIPCHK(c, upload_table(c->d_expo, c->expo));
  c->lmax = L;
  c->cstride = sh_chunk_stride(L);
  c->tables_dirty = false;
  c->quad_dirty = true;  // the cos/sin(m psi) table of shpair_upload_quadrature is sized by lmax
  return SHPAIR_OK;
}

// Uploads whatever table is stale (blocking copies): what a compute does on demand, callable ahead of a stream
// capture in which such copies are not allowed (shstep_run_device).
int shpair_prepare_tables(shpair_ctx* c)
{
  HIPCHK(c, hipSetDevice(c->device));
  if (c->tables_dirty) RC(upload_tables(c));
  if (c->quad_dirty) RC(shpair_upload_quadrature(c));
  HIPCHK(c, shp_size_pair_buffers(c, (size_t)c->npairs));
  return SHPAIR_OK;
}

extern "C" {

int shpair_settings(shpair_ctx* c, int nq)
{
  if (!c) return SHPAIR_EINVAL;
  if (nq < 1) CTX_FAIL(c, SHPAIR_EINVAL, "pair_style sh: nq must be >= 1 (got %d)", nq);
  if (nq > SHPAIR_MAX_NQ) CTX_FAIL(c, SHPAIR_ELMAX, "pair_style sh: nq %d > %d", nq, SHPAIR_MAX_NQ);
  c->nq = nq;
  c->quad_dirty = true;
  return SHPAIR_OK;
}

int shpair_set_ntypes(shpair_ctx* c, int ntypes, int nshapes)
{
  if (!c) return SHPAIR_EINVAL;
  if (ntypes < 1 || nshapes < 1) CTX_FAIL(c, SHPAIR_EINVAL, "ntypes (%d) and nshapes (%d) must be >= 1", ntypes, nshapes);
  c->ntypes = ntypes;
  c->nshapes = nshapes;
  c->shapes.assign(nshapes, Shape());
  c->mass_dirty = true;
  c->kn.assign((size_t)(ntypes + 1) * (ntypes + 1), std::nan(""));
  c->expo.assign((size_t)(ntypes + 1) * (ntypes + 1), std::nan(""));
  c->damp_gamma.clear();   // the damping coefficients go with the type table
  c->damp_on = false;
  c->fric_coef.clear();    // ... and so do the friction coefficients
  c->fric_on = false;
  c->spring_kt.clear();    // ... and the tangential springs, with what they hold
  c->hist_on = false;
  c->hist_np = -1;
  c->roll_coef.clear();    // ... and the rolling and twisting resistance
  c->twist_coef.clear();
  c->roll_on = c->twistres_on = false;
  c->integrals_src = nullptr;
  c->tables_dirty = true;
  return SHPAIR_OK;
}

int shpair_set_shape(shpair_ctx* c, int ishape, int lmax, const double* anm, double rmax)
{
  if (!c) return SHPAIR_EINVAL;
  if (c->nshapes <= 0) CTX_FAIL(c, SHPAIR_ESTATE, "shpair_set_ntypes() must come first");
  if (ishape < 0 || ishape >= c->nshapes) CTX_FAIL(c, SHPAIR_EINVAL, "shape index %d outside [0,%d)", ishape, c->nshapes);
  if (!anm) CTX_FAIL(c, SHPAIR_EINVAL, "null coefficient pointer");
  if (lmax < 0) CTX_FAIL(c, SHPAIR_EINVAL, "lmax %d < 0", lmax);
  if (lmax > SHPAIR_MAX_LMAX) CTX_FAIL(c, SHPAIR_ELMAX, "lmax %d > %d", lmax, SHPAIR_MAX_LMAX);
  const int n = (lmax + 1) * (lmax + 2);
  for (int k = 0; k < n; ++k)
    if (!std::isfinite(anm[k])) CTX_FAIL(c, SHPAIR_EINVAL, "shape %d: coefficient %d is not finite", ishape, k);
  Shape& s = c->shapes[ishape];
  s.lmax = lmax;
  s.anm.assign(anm, anm + n);
  // The bounding radius is a HARD bound in the algorithm (bounding-sphere reject, cap angle, LAMMPS' cutoff): an
  // underestimate silently drops contacts.  The default is 1.01 x the maximum over a sample grid (docs/SPEC.md §1);
  // the maximum between the samples is found by a local search from the best nodes, and a radius below it is refused.
  const double rtrue = refined_max_radius(lmax, anm);
  const double rdef = default_rmax(lmax, anm);
  // rtrue is itself a rounded host evaluation: an exactly tight user bound (a sphere's a00 / sqrt(4 pi), say) may land an
  // ulp below it, and a shortfall of 1e-12 relative cannot drop a contact
  if (rmax > 0.0 && rmax < rtrue * (1.0 - 1e-12))
    CTX_FAIL(c, SHPAIR_EINVAL, "shape %d: the bounding radius %.17g is below the shape's largest radius %.17g", ishape, rmax, rtrue);
  if (!(rmax > 0.0) && rdef < rtrue)
    CTX_FAIL(c, SHPAIR_EINVAL, "shape %d: the default bounding radius %.17g (1.01 x the sampled maximum) is below the largest "
             "radius %.17g found between the samples; pass an explicit rmax", ishape, rdef, rtrue);
  s.rmax = (rmax > 0.0) ? rmax : rdef;
  if (!(s.rmax > 0.0) || !std::isfinite(s.rmax)) CTX_FAIL(c, SHPAIR_EINVAL, "shape %d: bounding radius %g is not positive", ishape, s.rmax);
  c->tables_dirty = true;
  c->mass_dirty = true;
  return SHPAIR_OK;
}

int shpair_set_coeff(shpair_ctx* c, int itype, int jtype, double kn, double exponent)
{
  if (!c) return SHPAIR_EINVAL;
  if (c->ntypes <= 0) CTX_FAIL(c, SHPAIR_ESTATE, "shpair_set_ntypes() must come first");
  if (itype < 1 || itype > c->ntypes || jtype < 1 || jtype > c->ntypes)
    CTX_FAIL(c, SHPAIR_EINVAL, "pair_coeff types %d %d outside [1,%d]", itype, jtype, c->ntypes);
  if (!(kn >= 0.0) || !std::isfinite(kn)) CTX_FAIL(c, SHPAIR_EINVAL, "pair_coeff: kn %g must be finite and >= 0", kn);
  if (!(exponent >= 1.0) || !std::isfinite(exponent)) CTX_FAIL(c, SHPAIR_EINVAL, "pair_coeff: exponent %g must be finite and >= 1", exponent);
  c->kn[(size_t)itype * (c->ntypes + 1) + jtype] = kn;
  c->expo[(size_t)itype * (c->ntypes + 1) + jtype] = exponent;
  c->tables_dirty = true;
  return SHPAIR_OK;
}

int shpair_get_rmax(const shpair_ctx* c, int ishape, double* rmax)
{
  if (!c || !rmax) return SHPAIR_EINVAL;
  if (ishape < 0 || ishape >= c->nshapes || c->shapes[ishape].lmax < 0) return SHPAIR_EINVAL;
  *rmax = c->shapes[ishape].rmax;
  return SHPAIR_OK;
}

int shpair_shape_radius(int lmax, const double* anm, const double* u, double* r)
{
  if (lmax < 0 || lmax > SHPAIR_MAX_LMAX || !anm || !u || !r) return SHPAIR_EINVAL;
  *r = host_radius(lmax, anm, u);
  return SHPAIR_OK;
}

int shpair_shape_default_rmax(int lmax, const double* anm, double* rmax)
{
  if (lmax < 0 || lmax > SHPAIR_MAX_LMAX || !anm || !rmax) return SHPAIR_EINVAL;
  *rmax = default_rmax(lmax, anm);
  return SHPAIR_OK;
}

}  // extern "C"

// surface_state.hpp — the host state a surface pass keeps, once for the three families, planar walls (shstep_walls.hip),
// cylinders and cones (shell_host.hpp, for shstep_cylinders.hip and shstep_cones.hip): the work buffers, the
// tangential-spring history with the rules of its lifetime (SPEC §2.15, §2.19, §2.23) and the filler of the common kernel
// arguments.  Word is the mask word, W the doubles of xi per (particle, surface): 3 for a wall, 2 for a cylinder, 3 for a
// cone.  The pass, the setters and when the buffers are sized are shstep_walls.hip's for the walls and shell_host.hpp's
// for the two axial families.  Needs no kernel header.
#pragma once
#include <vector>

#include "shpair_ctx.hpp"
#include "surface_history.hpp"

struct shstep_state;

namespace shp {

// the buffers of a pass over nlocal particles; they only grow, so a caller that captures the pass sizes them first
template <typename Word>
struct SurfaceWork {
  DevBuf<Word> mask;           // [nlocal] surfaces within reach
  DevBuf<int> queue, count;    // [nlocal]; queue length, contacts
  DevBuf<double> rows, part;   // per-surface totals: rows of row_width, block sums
  hipError_t ensure(int nlocal, int nsurf, int row_width, bool want_out, int block)
  {
    const size_t n = nlocal > 0 ? (size_t)nlocal : 1;
    hipError_t e = mask.ensure(n);
    if (e == hipSuccess) e = queue.ensure(n);
    if (e == hipSuccess) e = count.ensure(2);
    if (e == hipSuccess && want_out) e = rows.ensure((size_t)row_width * n * (size_t)nsurf);
    if (e == hipSuccess && want_out) e = part.ensure((size_t)row_width * (size_t)nblk(nlocal, block) * (size_t)nsurf);
    return e;
  }
};

// xi per (particle, surface) and one live word per particle, keyed by the row index: rows of another nlocal hold nothing
// for the particles of a pass.  `what` is "wall" / "cylinder" / "cone", `setter` the spring's setter (for the messages).
template <typename Word, int W>
struct SurfaceHistory {
  DevBuf<double> xi;     // [nlocal][nsurf][W]; never zeroed: a dead bit reads as 0
  DevBuf<Word> live;     // [nlocal] one bit per surface whose xi is live
  int nlocal = -1;       // the rows xi / live are keyed by (the last advancing pass' or set's); -1: nothing live

  hipError_t size(int n_, int nsurf)   // growing drops what they held, which a changed nlocal does anyway
  {
    const size_t n = n_ > 0 ? (size_t)n_ : 1;
    if (W * n * (size_t)nsurf > xi.cap || n > live.cap) nlocal = -1;
    const hipError_t e = xi.ensure(W * n * (size_t)nsurf);
    return e == hipSuccess ? live.ensure(n) : e;
  }
  // ahead of a capture, the buffers sized: starts the rows of n_ particles from nothing live (blocks)
  int bind(shpair_ctx* c, int n_)
  {
    HIPCHK(c, hipDeviceSynchronize());   // an enqueued pass may still use the words
    HIPCHK(c, hipMemset(live.p, 0, (size_t)n_ * sizeof(Word)));
    nlocal = n_;
    return SHPAIR_OK;
  }
  // the prologue of a pass: rows keyed by another nlocal hold nothing for these particles, so an advancing pass starts
  // them from nothing live on its stream (the run loop did so ahead of its capture), a look reads every word as 0
  int begin_pass(shpair_ctx* c, int n_, bool advance, hipStream_t st, int* live_dead)
  {
    if (nlocal == n_) return SHPAIR_OK;
    if (!advance) {
      *live_dead = 1;
      return SHPAIR_OK;
    }
    HIPCHK(c, hipMemsetAsync(live.p, 0, (size_t)n_ * sizeof(Word), st));
    nlocal = n_;
    return SHPAIR_OK;
  }
  // xi to the host, 0 where the bit is dead (blocks); `on`: a spring is set
  int copy_out(shpair_ctx* c, const char* what, const char* setter, bool on, int n_, int nsurf, double* xi_out) const
  {
    if (!on) CTX_FAIL(c, SHPAIR_ESTATE, "copy %s history: no %s tangential spring is set (%s)", what, what, setter);
    if (n_ < 0 || (nlocal >= 0 && n_ != nlocal))
      CTX_FAIL(c, SHPAIR_EINVAL, "copy %s history: nlocal %d, the history is held for %d rows", what, n_, nlocal);
    if (n_ == 0) return SHPAIR_OK;
    if (!xi_out) CTX_FAIL(c, SHPAIR_EINVAL, "copy %s history: null output pointer", what);
    const size_t n = (size_t)n_, ns = (size_t)nsurf;
    for (size_t k = 0; k < W * n * ns; ++k) xi_out[k] = 0.0;
    if (nlocal < 0) return SHPAIR_OK;   // nothing live
    std::vector<double> h(W * n * ns);
    std::vector<Word> lv(n);
    HIPCHK(c, hipDeviceSynchronize());   // a pass may still be in flight
    HIPCHK(c, hipMemcpy(h.data(), xi.p, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(lv.data(), live.p, n * sizeof(Word), hipMemcpyDeviceToHost));
    history_mask_dead<Word, W>(h.data(), lv.data(), n, ns, xi_out);
    return SHPAIR_OK;
  }
  // xi from the host (a restart; blocks); size_buffers is the family's step_size_*_buffers, called once the device is idle
  int set_from_host(shpair_ctx* c, shstep_state* s, const char* what, const char* setter, bool on, int n_, int nsurf, const double* xi_in,
                    int (*size_buffers)(shpair_ctx*, shstep_state*, int, bool))
  {
    if (!on) CTX_FAIL(c, SHPAIR_ESTATE, "set %s history: no %s tangential spring is set (%s)", what, what, setter);
    if (n_ <= 0) CTX_FAIL(c, SHPAIR_EINVAL, "set %s history: nlocal %d < 1", what, n_);
    if (!xi_in) CTX_FAIL(c, SHPAIR_EINVAL, "set %s history: null array pointer", what);
    const size_t n = (size_t)n_, ns = (size_t)nsurf;
    std::vector<Word> lv(n);
    size_t bi = 0, bs = 0;
    if (!history_live_words<Word, W>(xi_in, n, ns, lv.data(), &bi, &bs))
      CTX_FAIL(c, SHPAIR_EINVAL, "set %s history: particle %zu, %s %zu: a number that is not finite", what, bi, what, bs);
    HIPCHK(c, hipDeviceSynchronize());
    RC(size_buffers(c, s, n_, false));
    HIPCHK(c, hipMemcpy(xi.p, xi_in, W * n * ns * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(live.p, lv.data(), n * sizeof(Word), hipMemcpyHostToDevice));
    nlocal = n_;
    return SHPAIR_OK;
  }
  int reset(shpair_ctx* c)
  {
    HIPCHK(c, hipDeviceSynchronize());   // an enqueued pass may still use the words
    nlocal = -1;                         // nothing to zero: the next pass starts from nothing live
    return SHPAIR_OK;
  }
};

// the common kernel arguments: P is a SurfaceParams (surface_pass.hpp), lay the context's QuadLayout (ring_tables.hpp)
template <typename Params, typename Layout, typename Word>
inline void fill_surface_params(Params& P, const shpair_ctx* c, const Layout& lay, int nlocal, int nsurf, const double* surf,
                                const double* x, const double* quat, const int* shtype, const int* mask, int groupbit, double* f,
                                double* torque, const SurfaceWork<Word>& work, bool want_rows)
{
  P.nlocal = nlocal; P.nsurf = nsurf; P.surf = surf;
  P.x = x; P.quat = quat; P.shtype = shtype; P.mask = mask; P.groupbit = groupbit; P.f = f; P.torque = torque;
  P.rc = c->d_rc.p; P.cw = c->d_coef.p; P.rmax = c->d_rmax.p; P.cstride = c->cstride; P.lmax = c->lmax; P.nshapes = c->nshapes;
  const double* q = c->d_quad.p;
  P.nq = c->nq; P.glt = q + lay.glt; P.glw = q + lay.glw; P.cpsi = q + lay.cpsi; P.spsi = q + lay.spsi;
  P.smask = work.mask.p; P.queue = work.queue.p; P.count = work.count.p; P.err = c->d_err.p;
  P.rows = want_rows ? work.rows.p : nullptr;
}

}  // namespace shp

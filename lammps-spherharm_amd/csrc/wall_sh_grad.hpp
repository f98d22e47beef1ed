// wall_sh_grad.hpp — r_i and the gradient of its polynomial extension from the recurrence tables of sh_device.hpp, rolled
// over (m, n): what the wall kernels of every surface evaluate per node (wall_kernels.hpp: planes, SPEC §2.9;
// cylinder_kernels.hpp: cylinders, §2.18).  One function, moved here word for word from wall_kernels.hpp; every planar
// wall kernel keeps its machine code.
#pragma once
#include <hip/hip_runtime.h>

#include "sh_device.hpp"

namespace shp {

// r and the Cartesian gradient of its polynomial extension  r = sum_m Re[W_m(z) (x + i y)^m]  at the unit vector
// (x, y, z).  Only the tangential part of the gradient is used, which no extension changes.
__device__ __forceinline__ void wall_sh_grad(const double* rc_in, const double* cw_in, const int LL, const double x,
                                             const double y, const double z, double& r, double& gx, double& gy, double& gz)
{
  double Cm = 1.0, Sm = 0.0, Cp = 0.0, Sp = 0.0;   // (x + i y)^m and ^(m-1)
  r = gx = gy = gz = 0.0;
#pragma unroll 1
  for (int m = 0; m <= LL; ++m) {
    const int o = sh_moff(LL, m);
    const cdptr rc = launder_uniform(rc_in + o);
    const cdptr cw = launder_uniform(cw_in + 2 * o);
    double Wr = cw[0], Wi = cw[1], Dr = 0.0, Di = 0.0;   // W_m and dW_m/dz
    if (m + 1 <= LL) {
      const double a1 = rc[1];
      double p2 = 1.0, d2 = 0.0;
      double p1 = a1 * z, d1 = a1;
      Wr = fma(cw[2], p1, Wr);
      Wi = fma(cw[3], p1, Wi);
      Dr = cw[2] * d1;
      Di = cw[3] * d1;
      for (int n = m + 2; n <= LL; ++n) {
        const int k = n - m;
        const double a = rc[k];
        const double p = fma(a, z * p1, -p2);
        const double d = fma(a, fma(z, d1, p1), -d2);
        Wr = fma(cw[2 * k], p, Wr);
        Wi = fma(cw[2 * k + 1], p, Wi);
        Dr = fma(cw[2 * k], d, Dr);
        Di = fma(cw[2 * k + 1], d, Di);
        p2 = p1; p1 = p;
        d2 = d1; d1 = d;
      }
    }
    r = fma(Wr, Cm, fma(-Wi, Sm, r));
    gz = fma(Dr, Cm, fma(-Di, Sm, gz));
    const double dm = (double)m;
    gx = fma(dm, fma(Wr, Cp, -(Wi * Sp)), gx);
    gy = fma(-dm, fma(Wr, Sp, Wi * Cp), gy);
    Cp = Cm;
    Sp = Sm;
    Cm = fma(Cp, x, -(Sp * y));
    Sm = fma(Cp, y, Sp * x);
  }
}

}  // namespace shp

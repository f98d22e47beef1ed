// contact_laws.hpp — the contact laws of docs/SPEC.md §2.10–§2.17 that more than one kernel body applies, once each.
//
// Device functions only, all inlined: no kernel, no kernel-argument struct, no state.  The callers are the pair slot
// body (dissipation_kernels.hpp, all six instances), the rolling slot (rolling_kernels.hpp), the wall rolling row
// (wall_roll_kernels.hpp), the axial roll row (shell_roll_kernels.hpp) and the three surface bodies (wall_kernels.hpp,
// cylinder_kernels.hpp, cone_kernels.hpp: pressure and viscous cap).
// Operand order, fma or plain form, the place of every sqrt and division and the sense of every comparison (a NaN takes
// the branch it takes) are part of a law.
// Every caller compiles to the machine code it had with the text written out.  Not here, because no form tried kept
// pair_damp_kernel's code (local vectors by pointer, by array reference, as scalars): the arm A = T_n - d x S_n and
// the nine-fma Vdot, which are text in pair_slot and in rolling_slot and must change together.
// The wall contact kernel (wall_kernels.hpp) has its own contact point: body-frame sums, the exact normal (no division
// by q).  Its pressure is pair_pressure inside `V > 0`, where the compiler drops the second test.
#pragma once
#include <hip/hip_runtime.h>

namespace shp {

// p = dE/dV = kn m V^(m-1); pow only where the exponent is not 1 (a slot touched with V <= 0 takes kn)
__device__ __forceinline__ double pair_pressure(const double kn, const double m, const double V)
{
  return (m == 1.0 || !(V > 0.0)) ? kn : kn * m * pow(V, m - 1.0);
}

// the Coulomb-capped viscous coefficient: g while g n <= cap, cap / n beyond (n = 0 takes the first branch)
__device__ __forceinline__ double capped_coefficient(const double g, const double n, const double cap)
{
  return g * n <= cap ? g : cap / n;
}

// The rolling and the twisting couple (SPEC §2.16, §2.17) under the normal load N > 0: Om is the relative angular
// velocity and On its part along the normal, which each caller forms its own way ((Om.S) S / q for a pair, (Om.n) n at a
// wall).  M = -kappa_r Om_r - kappa_tw On with either coefficient capped at mu N / |.| where its kind is on, 0 where it
// is off.  ADD: M is added to what is there (a wall row sums over its walls) instead of stored (0 + M would turn a -0
// into +0).  Returns the power kappa_r |Om_r|^2 + kappa_tw |On|^2.
template <bool ADD>
__device__ __forceinline__ double resisting_couples(const double* Om, const double* On, const double N, const bool roll, const double mur,
                                                    const double gr, const bool twst, const double mutw, const double gtw, double* M)
{
  const double Or[3] = {Om[0] - On[0], Om[1] - On[1], Om[2] - On[2]};
  const double nn2 = On[0] * On[0] + On[1] * On[1] + On[2] * On[2];
  const double nr2 = Or[0] * Or[0] + Or[1] * Or[1] + Or[2] * Or[2];
  double kr = 0.0, ktw = 0.0;
  if (roll) kr = capped_coefficient(gr, sqrt(nr2), mur * N);
  if (twst) ktw = capped_coefficient(gtw, sqrt(nn2), mutw * N);
  for (int k = 0; k < 3; ++k) {
    if constexpr (ADD) M[k] += -kr * Or[k] - ktw * On[k];
    else M[k] = -kr * Or[k] - ktw * On[k];
  }
  return kr * nr2 + ktw * nn2;
}

// omega_i - Omega a with the product rounded before the difference: no fma, so that a particle carried rigidly round by a
// shell that turns about its axis, omega_i = Omega a, has exactly 0 (SPEC §2.21, §2.24: the two axial roll rows)
__device__ __forceinline__ double relative_spin(const double om, const double O, const double a)
{
#pragma clang fp contract(off)
  const double carried = O * a;
  return om - carried;
}

// the slot's share of the energy tally (SPEC §2.13): 1 with newton_pair, else a half for i and a half for an owned j
__device__ __forceinline__ double ledger_share(const int newton_pair, const int j, const int nlocal)
{
  return newton_pair ? 1.0 : (0.5 + (j < nlocal ? 0.5 : 0.0));
}

}  // namespace shp

// rigid_body.hpp — what the kernels of step_kernels.hpp and dissipation_kernels.hpp share: the per-shape rigid-body row,
// the rotation matrix of a quaternion, the angular velocity of a body, and the error bit of a bad shape index.
#pragma once
#include <hip/hip_runtime.h>

namespace shp {

constexpr int kMassStride = 16;  // doubles per shape row: m, 1/m, c[3], Iinv (xx,yy,zz,xy,xz,yz), rmax, pad

// device error flags (shstep_state::d_flags[0]), read back at the blocking calls
constexpr int kErrShape = 1;  // shape index outside the table

struct Mat3 {
  double m[3][3];
};

__device__ inline Mat3 rot_of(const double w, const double x, const double y, const double z)
{
  Mat3 R;
  R.m[0][0] = w * w + x * x - y * y - z * z; R.m[0][1] = 2 * (x * y - w * z); R.m[0][2] = 2 * (x * z + w * y);
  R.m[1][0] = 2 * (x * y + w * z); R.m[1][1] = w * w - x * x + y * y - z * z; R.m[1][2] = 2 * (y * z - w * x);
  R.m[2][0] = 2 * (x * z - w * y); R.m[2][1] = 2 * (y * z + w * x); R.m[2][2] = w * w - x * x - y * y + z * z;
  return R;
}

// omega = R Iinv R^T L
__device__ inline void omega_of(const Mat3& R, const double* __restrict__ mr, const double L[3], double w[3])
{
  double lb[3], wb[3];
  for (int k = 0; k < 3; ++k) lb[k] = R.m[0][k] * L[0] + R.m[1][k] * L[1] + R.m[2][k] * L[2];
  wb[0] = mr[5] * lb[0] + mr[8] * lb[1] + mr[9] * lb[2];
  wb[1] = mr[8] * lb[0] + mr[6] * lb[1] + mr[10] * lb[2];
  wb[2] = mr[9] * lb[0] + mr[10] * lb[1] + mr[7] * lb[2];
  for (int k = 0; k < 3; ++k) w[k] = R.m[k][0] * wb[0] + R.m[k][1] * wb[1] + R.m[k][2] * wb[2];
}

}  // namespace shp

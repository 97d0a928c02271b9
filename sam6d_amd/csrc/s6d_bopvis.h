// The BOP19 visibility statement that VSD (csrc/s6d_boperr.hip, vsd_counts_kernel) and the ground-truth derivation
// (csrc/s6d_bopgt.hip, gt_visibility_kernel) share: ONE copy, so a ground-truth pixel is visible to both under the same float32
// operations.  Every operation is rounded on its own (contraction off inside each function; `/` and sqrtf correctly rounded).
// Likewise the vertex transform of the pose errors: MSSD / MSPD (csrc/s6d_boperr.hip) and ADD / ADD-S (csrc/s6d_adderr.hip).
#pragma once
#include "s6d_common.h"

namespace s6d {

// r = sqrtf((a a + b b) + 1),  a = ((float)u - cx) / fx,  b = ((float)v - cy) / fy:  D = Z r is the distance from the camera centre
__device__ __forceinline__ float bop_ray_factor(int u, int v, float fx, float fy, float cx, float cy) {
#pragma clang fp contract(off)
  const float a = ((float)u - cx) / fx, b = ((float)v - cy) / fy;
  return sqrtf((a * a + b * b) + 1.0f);
}

// vis_gt = Zg > 0 && ((Dg - Dt) <= delta || Zt == 0)
__device__ __forceinline__ bool bop_visible(float zg, float zt, float Dg, float Dt, float delta) {
#pragma clang fp contract(off)
  return zg > 0.f && ((Dg - Dt) <= delta || zt == 0.f);
}

// X = ((r00 vx + r01 vy) + r02 vz) + tx,  Y and Z alike, for the pose rows P = (r00 r01 r02 tx; r10 ...): the rasteriser's vertex statement
__device__ __forceinline__ void pose_err_transform(const float *__restrict__ P, float vx, float vy, float vz, float &X, float &Y,
                                                   float &Z) {
#pragma clang fp contract(off)
  X = ((P[0] * vx + P[1] * vy) + P[2] * vz) + P[3];
  Y = ((P[4] * vx + P[5] * vy) + P[6] * vz) + P[7];
  Z = ((P[8] * vx + P[9] * vy) + P[10] * vz) + P[11];
}

}  // namespace s6d

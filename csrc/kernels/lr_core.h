// Logistic regression on f32 feature values in the 16-row tile layout (4 lanes a row, lane
// group g holds features 8g .. 8g+7): the launch kernels on f32 rows (score_lr.hip) and the
// persistent kernel (score_persist.hip, f32 and W64 rows).  The W64 launch kernels use the
// folded weights of LrWireScorer (score_lr.hip), a different formula.
#pragma once
#include "common.h"

namespace ccfd {

constexpr int kLrBlob = 448;      // header 64, then mu, 1/sigma and w as 32 floats each

// Lane group g's share of the blob (models/lr.py pack).
struct LrLane {
  float mu[8], isg[8], w[8];
  float b;
  bool log_amount;
};

// `blob`: global memory, or a workgroup's LDS copy of it.
__device__ __forceinline__ LrLane lr_lane(const char* blob, int g) {
  LrLane L;
  L.log_amount = (*reinterpret_cast<const unsigned*>(blob + 4) & 1u) != 0;
  L.b = *reinterpret_cast<const float*>(blob + 8);
  const float* mu = reinterpret_cast<const float*>(blob + 64) + 8 * g;
  const float* isg = reinterpret_cast<const float*>(blob + 192) + 8 * g;
  const float* w = reinterpret_cast<const float*>(blob + 320) + 8 * g;
#pragma unroll
  for (int j = 0; j < 8; ++j) { L.mu[j] = mu[j]; L.isg[j] = isg[j]; L.w[j] = w[j]; }
  return L;
}

// proba_1 of row (lane & 15) from this lane's 8 features: 8 FMAs per lane plus two
// xor-shuffles over the row's 4 lanes.  The g == 3 lanes carry Time and Amount and no features
// 6 / 7; xv[5] (Amount) is replaced by its log1p when the model asks for it.
__device__ __forceinline__ float lr_proba(const LrLane& L, float (&xv)[8], int g) {
  if (g == 3) {
    xv[6] = 0.f; xv[7] = 0.f;
    if (L.log_amount) xv[5] = log1pf(fmaxf(xv[5], 0.f));
  }
  float z = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) z = fmaf((xv[j] - L.mu[j]) * L.isg[j], L.w[j], z);
  z += __shfl_xor(z, 16);
  z += __shfl_xor(z, 32);
  return sigmoid(z + L.b);
}

}  // namespace ccfd

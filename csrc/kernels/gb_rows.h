// 64-row chunk staging shared by the tree scorers (score_gbdt.hip v1, score_forest.hip):
// contiguous f32 rows -> registers (prefetch) -> feature-major LDS tile xs[30][64].
#pragma once
#include "common.h"

namespace ccfd {

constexpr int kGbRows = 64;
constexpr int kGbWaves = 4;
constexpr int kGbF4 = kGbRows * kF / 4;   // 480 float4 per 64-row chunk

// Register-staged copy of one 64-row chunk (contiguous rows): thread t owns float4 t and
// t + 256 of the chunk's 7680 bytes.
struct GbRegs { float4 v[2]; };

__device__ __forceinline__ void gb_issue(const float* __restrict__ x, int row0, int nrows, int tid, GbRegs& r) {
  const int avail = nrows * kF * 4;
  const float4* src = reinterpret_cast<const float4*>(x + (size_t)row0 * kF);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int i = tid + 256 * k;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < kGbF4) {
      if (i * 16 + 16 <= avail) v = src[i];
      else if (i * 16 + 8 <= avail) { const float2 h = reinterpret_cast<const float2*>(src)[2 * i]; v.x = h.x; v.y = h.y; }
    }
    r.v[k] = v;
  }
}

__device__ __forceinline__ void gb_store(float (*xs)[kGbRows], int tid, const GbRegs& r) {
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int i = tid + 256 * k;
    if (i < kGbF4) {
      const int e = 4 * i;
      const float vv[4] = {r.v[k].x, r.v[k].y, r.v[k].z, r.v[k].w};
#pragma unroll
      for (int q = 0; q < 4; ++q) { const int ee = e + q; xs[ee % kF][ee / kF] = vv[q]; }
    }
  }
}

}  // namespace ccfd

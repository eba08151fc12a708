// The 64-row chunk frame shared by the tree scorers on f32 rows (score_gbdt.hip v1,
// score_forest.hip): contiguous rows -> registers (prefetch) -> feature-major LDS tile
// xs[30][64], or strided rows straight into the tile (gb_stage); and what wave 0 does with a
// chunk's 64 probabilities (gb_row_epilogue).
#pragma once
#include "common.h"
#include "rules.h"

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

// The chunk at row0 into xs.  Contiguous rows: the next chunk of the workgroup's run (if
// `more`) is issued into `nxt` first, then `cur` -- fetched while the previous chunk was
// scored -- is stored.  Strided rows: loaded here, rows past the batch as zeros.
template <bool kContig>
__device__ __forceinline__ void gb_stage(const ccfd_score_args& a, float (*xs)[kGbRows], int tid, int row0, int nrows,
                                         bool more, const GbRegs& cur, GbRegs& nxt) {
  if constexpr (kContig) {
    if (more) gb_issue(a.x, row0 + kGbRows, min(kGbRows, a.n - row0 - kGbRows), tid, nxt);
    gb_store(xs, tid, cur);
  } else {
    for (int e = tid; e < kGbRows * kF; e += 256) {
      const int r = e / kF, f = e % kF;
      xs[f][r] = (r < nrows) ? a.x[(size_t)(row0 + r) * a.ld + f] : 0.f;
    }
  }
}

// Finish a row, by one wave: lane = row of the chunk, p its probability.  Threshold or the
// configurable routing rules (the row's features are column xs[*][lane]), the proba / route
// stores, the amount histogram, the workgroup's counters and the flag list.
template <bool kR>
__device__ __forceinline__ void gb_row_epilogue(const ccfd_score_args& a, EpilogueLds& epi, const float (*xs)[kGbRows],
                                                float p, int lane, int row0, int nrows) {
  const bool valid = lane < nrows;
  bool fr;
  if constexpr (kR) fr = valid && rule_route(a.rules, p, [&](int j) { return xs[j][lane]; });
  else fr = valid && (p >= a.threshold);
  const int row = row0 + lane;
  if (valid) {
    if (a.proba) st_g(a.proba + row, p);
    if (a.route) st_g(a.route + row, (uint8_t)(fr ? 1 : 0));
    atomicAdd(&epi.hist[(fr ? kNB : 0) + amount_bucket(xs[kAmountCol][lane])], 1u);
  }
  unsigned long long ps = valid ? (unsigned long long)(p * 1e6f + 0.5f) : 0ull;
  ps = wave_sum_u64(ps);
  const unsigned nf = __popcll(__ballot(fr));
  if (lane == 0) { epi.fraud += nf; epi.rows += nrows; epi.psum_e6 += ps; }
  emit_flagged(a, fr, row);
}

}  // namespace ccfd

// What every MLP / LR kernel does with a scored row of a 16-row tile (4 lanes a row: lane
// (g, c) holds 8 features of row c, the row's proba_1 is identical in the 4 lane groups):
// validity, route, proba / route outputs, the proba sum, fraud and row ballots and the amount
// histogram -- and how a wave's counts reach the workgroup's LDS accumulators.  Two forms:
//   tile_row_epilogue        owner lanes g == 0, one LDS histogram atomic per row: the f32-row
//                            launch kernels (score_mlp.hip, score_lr.hip) and the persistent
//                            kernels (score_persist.hip, score_shadow.hip);
//   tile_row_epilogue_lanes  fraud ballot on the g == 3 lanes (which hold the amount), the
//                            histogram in per-lane HistLanes counters: the W64 streaming bodies
//                            (wire_body.h, score_shadow.hip).
// The flag list stays with the caller (emit_flagged, flag_push and persist_emit_flagged are
// different protocols), as in g32_core.h for the binned-row kernels.
#pragma once
#include "common.h"

namespace ccfd {

// Per-wave counts of the rows scored so far (a launch: all of them; a persistent kernel: the
// wave's share of one item).
struct TileWave {
  unsigned fraud = 0, rows = 0;
  unsigned long long psum = 0;
};

struct TileRowOut {
  bool valid, fr;                // inside the batch; routed to fraud (in all 4 lanes of the row)
  unsigned long long m;          // __ballot of the fraud rows' owner lanes (g == 0, or g == 3 for _lanes)
};

// `p`: the row's proba_1.  `route_fr`: the routing decision -- p >= threshold, or the rule
// result the caller computed from the features it holds.  `amount`: the row's Amount as held by
// the g == 3 lanes.
__device__ __forceinline__ TileRowOut tile_row_epilogue(EpilogueLds& epi, TileWave& w, float p, bool route_fr,
                                                        float amount, int row, int n, int g, float* proba,
                                                        uint8_t* route) {
  const bool valid = row < n;
  const bool fr = valid && route_fr;
  if (valid && g == 0) {
    if (proba) st_g(proba + row, p);
    if (route) st_g(route + row, (uint8_t)(fr ? 1 : 0));
    w.psum += (unsigned)(p * 1e6f + 0.5f);              // p in [0,1]: u32 convert, u64 sum
  }
  const unsigned long long m = __ballot(fr && g == 0);
  w.fraud += __popcll(m);
  w.rows += __popcll(__ballot(valid && g == 0));
  if (valid && g == 3) atomicAdd(&epi.hist[(fr ? kNB : 0) + amount_bucket_fast(amount)], 1u);
  return TileRowOut{valid, fr, m};
}

// The HistLanes form, row c of tile `t`: every row into the lane-spread "amount > bound"
// counters, only fraud rows (rare) into the LDS histogram.
__device__ __forceinline__ TileRowOut tile_row_epilogue_lanes(EpilogueLds& epi, TileWave& w, HistLanes& hl, float p,
                                                              bool route_fr, float amount, int t, int n, int g, int c,
                                                              float* proba, uint8_t* route) {
  const int row = t * kTileRows + c;
  const bool valid = row < n;
  const bool fr = valid && route_fr;
  if (valid && g == 0) {
    if (proba) st_g(proba + row, p);
    if (route) st_g(route + row, (uint8_t)(fr ? 1 : 0));
    w.psum += (unsigned)(p * 1e6f + 0.5f);
  }
  const unsigned long long m = __ballot(fr && g == 3);          // same rows as the g == 0 lanes
  w.fraud += __popcll(m);
  w.rows += (unsigned)min(kTileRows, n - t * kTileRows);
  const float am_g3 = (valid && g == 3) ? amount : -__builtin_inff();
  hist_lanes_add(hl, __shfl(am_g3, 48 + c));
  if (m && fr && g == 3) atomicAdd(&epi.hist[kNB + amount_bucket_fast(amount)], 1u);   // rare: fraud rows' buckets
  return TileRowOut{valid, fr, m};
}

// Wave -> workgroup (LDS) at the end of a launch.
__device__ __forceinline__ void tile_wave_commit(EpilogueLds& epi, TileWave& w, int lane) {
  w.psum = wave_sum_u64(w.psum);
  if (lane == 0) {
    atomicAdd(&epi.fraud, w.fraud);
    atomicAdd(&epi.rows, w.rows);
    atomicAdd(&epi.psum_e6, w.psum);
  }
}

// The same at the end of a persistent item: a wave that had no rows of the item adds nothing,
// and the counts start over for the next item.
__device__ __forceinline__ void tile_item_commit(EpilogueLds& epi, TileWave& w, int lane) {
  w.psum = wave_sum_u64(w.psum);
  if (lane == 0 && w.rows) {
    atomicAdd(&epi.fraud, w.fraud);
    atomicAdd(&epi.rows, w.rows);
    atomicAdd(&epi.psum_e6, w.psum);
  }
  w = TileWave{};
}

}  // namespace ccfd

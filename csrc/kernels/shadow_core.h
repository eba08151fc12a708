// Counter accumulation of a shadow (challenger) model, shared by the shadow kernels
// (score_shadow.hip: MLP on W64 rows; score_gbdt_shadow.hip: oblivious GBDT on G32 / G20
// rows).  The five CCFD_CNT_SHADOW_* slots are accumulated per wave in registers, then per
// workgroup in LDS, then with one set of atomics per workgroup (launch kernels) or per item
// (persistent kernels).
#pragma once
#include "common.h"

namespace ccfd {

// Per-workgroup accumulators of the challenger's counters.
struct ShadowLds {
  unsigned int rows, fraud, both, pad;
  unsigned long long psum_e6, absdiff_e6;
};

struct ShadowAcc {                       // per wave, in registers
  unsigned fraud = 0, both = 0;
  unsigned long long psum = 0, absdiff = 0;
};

__device__ __forceinline__ void shadow_init(ShadowLds& s) {
  if (threadIdx.x == 64) { s.rows = 0; s.fraud = 0; s.both = 0; s.pad = 0; s.psum_e6 = 0; s.absdiff_e6 = 0; }
}

// One row's challenger bookkeeping, in the lane that owns the row's outputs.
__device__ __forceinline__ void shadow_row(ShadowAcc& w, float p, float q) {
  w.psum += (unsigned)(q * 1e6f + 0.5f);                 // the rounding of CCFD_CNT_PROBA_E6
  w.absdiff += (unsigned)(fabsf(p - q) * 1e6f + 0.5f);
}

// Wave -> workgroup: `rows` = valid rows this wave scored (wave-uniform).
__device__ __forceinline__ void shadow_wave_commit(ShadowLds& s, ShadowAcc& w, unsigned rows, int lane) {
  w.psum = wave_sum_u64(w.psum);
  w.absdiff = wave_sum_u64(w.absdiff);
  if (lane == 0 && rows) {
    atomicAdd(&s.rows, rows);
    atomicAdd(&s.fraud, w.fraud);
    atomicAdd(&s.both, w.both);
    atomicAdd(&s.psum_e6, w.psum);
    atomicAdd(&s.absdiff_e6, w.absdiff);
  }
}

// Workgroup -> global, one thread, after a barrier that follows every wave's commit.
__device__ __forceinline__ void shadow_flush(const ShadowLds& s, unsigned long long* cnt) {
  if (cnt == nullptr || s.rows == 0) return;
  atomicAdd(&cnt[CCFD_CNT_SHADOW_ROWS], (unsigned long long)s.rows);
  atomicAdd(&cnt[CCFD_CNT_SHADOW_FRAUD], (unsigned long long)s.fraud);
  atomicAdd(&cnt[CCFD_CNT_SHADOW_BOTH], (unsigned long long)s.both);
  atomicAdd(&cnt[CCFD_CNT_SHADOW_PROBA_E6], s.psum_e6);
  atomicAdd(&cnt[CCFD_CNT_SHADOW_ABSDIFF_E6], s.absdiff_e6);
}

}  // namespace ccfd

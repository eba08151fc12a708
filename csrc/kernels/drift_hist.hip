// Per-feature bin counts of G32 / G20 rows, for drift detection (models/drift.py holds the
// definition, the numpy oracle and PSI; ops/kernels.py drift_histogram / DriftMonitor).
//
// A binned row is the transaction discretised against the model's own split table, so a
// histogram of its bytes is the feature distribution at exactly the resolution the model can
// see.  For every row whose stamp equals args.stamp: counts[j][bin_j] += 1 (j < 30),
// counts[30][amount bucket] += 1, tail[0] += 1; a row with another stamp adds 1 to tail[1] and
// nothing else (what the scorers count in CCFD_CNT_WIRE_STALE).  The launch accumulates.
//
// One row per lane, held in registers (2 x 16 B for G32, 5 dwords for G20); the 30 bins are
// lifted with compile-time bit-field extracts (g32_core.h) and counted in a workgroup-private
// LDS table of u32 -- [31][256] = 31.7 KB for G32, [31][32] = 4 KB for G20 -- with no-return LDS
// integer adds.  Every bin value has a cell by construction (a byte has 256 values, 5 bits
// have 32; the 4-bit G20 bucket fits the 32-cell column), so no index depends on unchecked
// data.  Workgroups stride over the rows, then flush their non-zero cells with 64-bit global
// atomic adds, consecutive lanes taking consecutive cells.  Integer sums: exact and
// bit-reproducible whatever the grid.
#include <algorithm>
#include <string>

#include "g32_core.h"

namespace ccfd {

void set_error(const std::string& e);

constexpr int kDriftThreads = 256;
constexpr int kDriftRowsPerWg = 1024;        // fewer rows than this do not get their own workgroup
constexpr int kDriftCols = CCFD_DRIFT_COLS;  // 30 features + the amount bucket
constexpr int kDriftCells = CCFD_DRIFT_CELLS;

__device__ __forceinline__ void lds_inc(unsigned* p) {
  __hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <bool kG20>
__device__ __forceinline__ G32Row drift_row(const uint8_t* __restrict__ rows, int64_t i) {
  G32Row r;
  if constexpr (kG20) {
    const unsigned* __restrict__ w = reinterpret_cast<const unsigned*>(rows) + i * kG20Words;
    r.lo.x = ld_g(w);
    r.lo.y = ld_g(w + 1);
    r.lo.z = ld_g(w + 2);
    r.lo.w = ld_g(w + 3);
    r.hi = make_uint4(ld_g(w + 4), 0u, 0u, 0u);
  } else {
    r.lo = ld_g16(rows + i * CCFD_G32_ROW_BYTES);
    r.hi = ld_g16(rows + i * CCFD_G32_ROW_BYTES + 16);
  }
  return r;
}

// Workgroup blk counts rows blk * 256 + tid striding by gridDim.x * 256.
template <bool kG20>
__global__ __launch_bounds__(kDriftThreads) void drift_hist_kernel(ccfd_drift_hist_args a) {
  constexpr int C = kG20 ? 32 : kDriftCells;           // cells of one column in LDS
  __shared__ unsigned tab[kDriftCols * C];
  __shared__ unsigned tl[2];
  const int tid = threadIdx.x;
  for (int c = tid; c < kDriftCols * C; c += kDriftThreads) tab[c] = 0u;
  if (tid < 2) tl[tid] = 0u;
  __syncthreads();

  unsigned counted = 0, stale = 0;
  const int64_t stride = (int64_t)gridDim.x * kDriftThreads;
  for (int64_t i = (int64_t)blockIdx.x * kDriftThreads + tid; i < a.n; i += stride) {
    const G32Row r = drift_row<kG20>(a.rows, i);
    unsigned b[kF];
    const unsigned bs = gx_lift<kG20>(r, b);           // bucket | stamp << 8
    if ((bs >> 8) == (unsigned)a.stamp) {
#pragma unroll
      for (int j = 0; j < kF; ++j) lds_inc(tab + j * C + b[j]);
      lds_inc(tab + kF * C + (bs & 0xffu));
      ++counted;
    } else {
      ++stale;
    }
  }
  if (counted) __hip_atomic_fetch_add(&tl[0], counted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (stale) __hip_atomic_fetch_add(&tl[1], stale, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __syncthreads();

  // LDS cell c = (column, cell) -> counts[column][cell] of the [31][256] output
  for (int c = tid; c < kDriftCols * C; c += kDriftThreads) {
    const unsigned v = tab[c];
    if (v) atomicAdd(a.counts + (c / C) * kDriftCells + (c % C), (unsigned long long)v);
  }
  if (tid < 2 && tl[tid]) atomicAdd(a.tail + tid, (unsigned long long)tl[tid]);
}

}  // namespace ccfd

extern "C" int ccfd_drift_hist_launch(const ccfd_drift_hist_args* a, void* stream) {
  using namespace ccfd;
  if (a == nullptr || a->counts == nullptr || a->tail == nullptr || (a->rows == nullptr && a->n != 0)) {
    set_error("drift histogram: null argument");
    return -1;
  }
  const bool g20 = a->wire == (CCFD_ARG_WIRE_G32 | CCFD_ARG_WIRE_G20);
  if (!g20 && a->wire != CCFD_ARG_WIRE_G32) {
    set_error("drift histogram: wire must be CCFD_ARG_WIRE_G32 or CCFD_ARG_WIRE_G32 | CCFD_ARG_WIRE_G20");
    return -2;
  }
  if (a->n < 0) { set_error("drift histogram: n < 0"); return -2; }
  if (a->stamp < 1 || a->stamp > (g20 ? 63 : 255)) {
    set_error(g20 ? "drift histogram: G20 stamp outside 1..63" : "drift histogram: G32 stamp outside 1..255");
    return -2;
  }
  if (a->max_workgroups < 1) { set_error("drift histogram: max_workgroups < 1"); return -2; }
  if (reinterpret_cast<uintptr_t>(a->rows) & (g20 ? 3 : 15)) {
    set_error(g20 ? "drift histogram: G20 rows must be 4-byte aligned" : "drift histogram: G32 rows must be 16-byte aligned");
    return -3;
  }
  if ((reinterpret_cast<uintptr_t>(a->counts) | reinterpret_cast<uintptr_t>(a->tail)) & 7) {
    set_error("drift histogram: counts and tail must be 8-byte aligned");
    return -3;
  }
  if (a->n == 0) return 0;
  const int64_t by_rows = (a->n + kDriftRowsPerWg - 1) / kDriftRowsPerWg;
  const int grid = (int)std::min<int64_t>(a->max_workgroups, by_rows);
  // a workgroup's cells are u32: it must see fewer than 2^32 rows
  if ((a->n + grid - 1) / grid + kDriftThreads > (int64_t)0xffffffffll) {
    set_error("drift histogram: more than 2^32 rows a workgroup; raise max_workgroups or split the launch");
    return -2;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (g20) hipLaunchKernelGGL(drift_hist_kernel<true>, dim3(grid), dim3(kDriftThreads), 0, s, *a);
  else hipLaunchKernelGGL(drift_hist_kernel<false>, dim3(grid), dim3(kDriftThreads), 0, s, *a);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
    set_error(std::string("drift histogram: launch failed: ") + hipGetErrorString(e));
    return -5;
  }
  return 0;
}

// Per-feature quantile-bin counts of W64 rows, for drift detection on the MLP / LR path
// (models/drift.py holds the definition, the numpy oracle wire_bin_counts and PSI;
// ops/kernels.py drift_histogram_wire / DriftMonitor).
//
// A W64 row carries values, not bins (bf16 V1..V28, f32 Time, f32 Amount), so this kernel bins
// before it counts: for every row, counts[j][#{edges_j < x_j}] += 1 for the 30 features in
// canonical order (Time, V1..V28, Amount), counts[30][amount bucket] += 1 and tail[0] += 1.
// W64 rows carry no stamp, so tail[1] is never touched.  The launch accumulates.
//
// The edge table is float[30][32] in LDS: each feature's ascending edges, then +inf.  A +inf
// edge is below no value, so the padding never counts and the search below is a fixed
// five-step, branch-free lower bound over 32 entries whose result is 0..31 whatever the row
// holds: no LDS index depends on unchecked data.  The compare is the IEEE f32 `<` on the widened
// value (NaN -> cell 0, -0 == 0, denormals kept: the code object runs with f32 denormals on).
// One row per lane in registers (4 x 16 B); the 30 searches of a row are independent, so their
// dependent LDS reads overlap.  Cells are counted in a workgroup-private u32 [31][32] LDS table
// with no-return integer adds and flushed with 64-bit global atomic adds, as drift_hist.hip
// does.  Integer sums: exact and bit-reproducible whatever the grid.
#include <algorithm>
#include <string>

#include "common.h"

namespace ccfd {

void set_error(const std::string& e);

constexpr int kWireDriftThreads = 256;
constexpr int kWireDriftRowsPerWg = 1024;     // fewer rows than this do not get their own workgroup
constexpr int kWireDriftCols = CCFD_DRIFT_COLS;
constexpr int kWireDriftFeat = CCFD_DRIFT_COLS - 1;
constexpr int kWireDriftEdges = CCFD_DRIFT_WIRE_EDGES;   // 32: <= 31 edges + padding, and the LDS cells of a column

__device__ __forceinline__ void wire_lds_inc(unsigned* p) {
  __hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// #{e[k] < x} over the padded 32-entry row `e`: 0..31.
__device__ __forceinline__ unsigned wire_bin(const float* e, float x) {
  unsigned pos = 0;
#pragma unroll
  for (unsigned step = 16; step >= 1; step >>= 1) pos += (e[pos + step - 1] < x) ? step : 0u;
  return pos;
}

// Workgroup blk counts rows blk * 256 + tid striding by gridDim.x * 256.
__global__ __launch_bounds__(kWireDriftThreads) void drift_wire_kernel(ccfd_drift_wire_args a) {
  __shared__ float ed[kWireDriftFeat * kWireDriftEdges];
  __shared__ unsigned tab[kWireDriftCols * kWireDriftEdges];
  __shared__ unsigned tl;
  const int tid = threadIdx.x;
  for (int c = tid; c < kWireDriftFeat * kWireDriftEdges; c += kWireDriftThreads) ed[c] = ld_g(a.edges + c);
  for (int c = tid; c < kWireDriftCols * kWireDriftEdges; c += kWireDriftThreads) tab[c] = 0u;
  if (tid == 0) tl = 0u;
  __syncthreads();

  unsigned counted = 0;
  const int64_t stride = (int64_t)gridDim.x * kWireDriftThreads;
  for (int64_t i = (int64_t)blockIdx.x * kWireDriftThreads + tid; i < a.n; i += stride) {
    const uint8_t* __restrict__ p = a.rows + i * CCFD_WIRE_ROW_BYTES;
    const uint4 q[4] = {ld_g16(p), ld_g16(p + 16), ld_g16(p + 32), ld_g16(p + 48)};
    const unsigned w[16] = {q[0].x, q[0].y, q[0].z, q[0].w, q[1].x, q[1].y, q[1].z, q[1].w,
                            q[2].x, q[2].y, q[2].z, q[2].w, q[3].x, q[3].y, q[3].z, q[3].w};
    const float amount = __uint_as_float(w[15]);
    wire_lds_inc(tab + wire_bin(ed, __uint_as_float(w[14])));                        // Time
#pragma unroll
    for (int v = 0; v < 28; ++v) {                                                   // V1..V28, bf16 -> f32
      const float x = __uint_as_float((v & 1) ? (w[v >> 1] & 0xffff0000u) : (w[v >> 1] << 16));
      wire_lds_inc(tab + (v + 1) * kWireDriftEdges + wire_bin(ed + (v + 1) * kWireDriftEdges, x));
    }
    wire_lds_inc(tab + 29 * kWireDriftEdges + wire_bin(ed + 29 * kWireDriftEdges, amount));
    wire_lds_inc(tab + kWireDriftFeat * kWireDriftEdges + (unsigned)amount_bucket_fast(amount));   // 0..13
    ++counted;
  }
  if (counted) __hip_atomic_fetch_add(&tl, counted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __syncthreads();

  // LDS cell c = (column, cell) -> counts[column][cell] of the [31][256] output
  for (int c = tid; c < kWireDriftCols * kWireDriftEdges; c += kWireDriftThreads) {
    const unsigned v = tab[c];
    if (v) atomicAdd(a.counts + (c / kWireDriftEdges) * CCFD_DRIFT_CELLS + (c % kWireDriftEdges), (unsigned long long)v);
  }
  if (tid == 0 && tl) atomicAdd(a.tail, (unsigned long long)tl);
}

}  // namespace ccfd

extern "C" int ccfd_drift_wire_launch(const ccfd_drift_wire_args* a, void* stream) {
  using namespace ccfd;
  if (a == nullptr || a->edges == nullptr || a->counts == nullptr || a->tail == nullptr ||
      (a->rows == nullptr && a->n != 0)) {
    set_error("drift wire histogram: null argument");
    return -1;
  }
  if (a->n < 0) { set_error("drift wire histogram: n < 0"); return -2; }
  if (a->max_workgroups < 1) { set_error("drift wire histogram: max_workgroups < 1"); return -2; }
  if (reinterpret_cast<uintptr_t>(a->rows) & 15) {
    set_error("drift wire histogram: W64 rows must be 16-byte aligned");
    return -3;
  }
  if (reinterpret_cast<uintptr_t>(a->edges) & 3) {
    set_error("drift wire histogram: edges must be 4-byte aligned");
    return -3;
  }
  if ((reinterpret_cast<uintptr_t>(a->counts) | reinterpret_cast<uintptr_t>(a->tail)) & 7) {
    set_error("drift wire histogram: counts and tail must be 8-byte aligned");
    return -3;
  }
  if (a->n == 0) return 0;
  const int64_t by_rows = (a->n + kWireDriftRowsPerWg - 1) / kWireDriftRowsPerWg;
  const int grid = (int)std::min<int64_t>(a->max_workgroups, by_rows);
  // a workgroup's cells are u32: it must see fewer than 2^32 rows
  if ((a->n + grid - 1) / grid + kWireDriftThreads > (int64_t)0xffffffffll) {
    set_error("drift wire histogram: more than 2^32 rows a workgroup; raise max_workgroups or split the launch");
    return -2;
  }
  hipLaunchKernelGGL(drift_wire_kernel, dim3(grid), dim3(kWireDriftThreads), 0, reinterpret_cast<hipStream_t>(stream), *a);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
    set_error(std::string("drift wire histogram: launch failed: ") + hipGetErrorString(e));
    return -5;
  }
  return 0;
}

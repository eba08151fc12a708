// G32 / G20 oblivious-GBDT scorer, one launch per micro-batch (engine exec_mode = 0, score_sync).
// Row format, level form and layout: g32_core.h; persistent variant: score_gbdt_g32_persist.hip.
#include "g32_core.h"

namespace ccfd {

template <int D, int R, bool kR, bool kGL, bool kG20>
__global__ __launch_bounds__(256) void score_gbdt_g32_kernel(ccfd_score_args a) {
  extern __shared__ __attribute__((aligned(16))) float lv[];   // T * L floats
  __shared__ uint4 xt[kG32Waves][128];                         // per-wave chunk transpose
  __shared__ EpilogueLds epi;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = a.n;
  const int nchunks = (n + kG32Rows - 1) / kG32Rows;
  const int ngroups = (nchunks + R - 1) / R;                  // R chunks per wave step
  const int gstride = gridDim.x * kG32Waves;
  int grp = blockIdx.x * kG32Waves + wave;
  const unsigned char* __restrict__ xb = reinterpret_cast<const unsigned char*>(a.x);

  // rows first: the host-memory latency overlaps the leaf staging below
  G32Row pre[R];
#pragma unroll
  for (int q = 0; q < R; ++q) gx_fetch<kG20>(xb, n, grp * R + q, lane, pre[q]);

  epi_init(epi);
  stamp_start(a, blockIdx.x);
  const int T = a.gbdt_trees;
  const G32Model M = g32_model<D>(a.blob, T);
  const float* leaves = g32_leaves<D, kGL>(M, T, lv, tid, 256);
  __syncthreads();                                              // leaves staged, epi initialised

  G32Wave w;
  for (; grp < ngroups; grp += gstride) {
    // separate 1-D arrays per row chain: indexed by a runtime (wave-uniform) feature id they
    // stay in VGPRs (v_movrel); a 2-D array would be demoted to scratch
    unsigned b0[kF], b1[kF];
    unsigned meta[R];                                           // bucket | stamp << 8
    G32Row cur = pre[0];
    gx_rows<kG20>(xt[wave], lane, cur);
    meta[0] = gx_lift<kG20>(cur, b0);
    if constexpr (R == 2) {
      cur = pre[1];
      gx_rows<kG20>(xt[wave], lane, cur);
      meta[1] = gx_lift<kG20>(cur, b1);
    }
    const int nxt = grp + gstride;
    if (nxt < ngroups) {
#pragma unroll
      for (int q = 0; q < R; ++q) gx_fetch<kG20>(xb, n, nxt * R + q, lane, pre[q]);
    }
    float acc[R];
    g32_trees<D, R>(b0, b1, leaves, M.feat, M.kbin, T, acc);
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int row = (grp * R + q) * kG32Rows + lane;
      const G32RowOut o = g32_row_epilogue<kR>(epi, w, M, meta[q], acc[q], row, n, a.threshold, a.rules, a.proba, a.route);
      emit_flagged(a, o.fr, row);
    }
  }
  g32_wave_commit(epi, w, a.counters, lane);
  epi_flush(epi, a.counters);
  signal_done(a, gridDim.x);
}

// Grid: one wave per R-chunk group, capped at CCFD_G32_WGS_PER_CU workgroups per CU (grid-
// stride beyond).  A 65536-row micro-batch is 1024 chunks = 256 workgroups at R = 1: every
// CU has its rows in flight at once.  CCFD_G32_R: 64-row chunks per wave step (1 | 2).
template <int D, int R, bool kG20>
static void launch_g32_r(const ccfd_score_args& a, hipStream_t s) {
  constexpr int L = 1 << D;
  const int wgs_per_cu = g32_env("CCFD_G32_WGS_PER_CU", 4, 1, 8);   // read per launch: sweepable in-process
  const int nchunks = (a.n + kG32Rows - 1) / kG32Rows;
  const int ngroups = (nchunks + R - 1) / R;
  int grid = (ngroups + kG32Waves - 1) / kG32Waves;
  const int cap = 256 * wgs_per_cu;
  grid = grid < 1 ? 1 : (grid > cap ? cap : grid);
  // a launch re-stages the leaves in every workgroup: past 32 KB of leaves the L2 gather wins
  // (250 x 6 at 1 M rows: 5.3 vs 4.0 G rows/s; 100 x 6: LDS 14.2 vs 13.1 at 16 M rows,
  // profiles/r2/g32_large_ensembles/lds_vs_global_*.jsonl)
  const bool gl = ((long)a.gbdt_trees << D) > kG32LeafLds / 2 || g32_env("CCFD_G32_GLOBAL_LEAVES", 0, 0, 1);
  const size_t lds = gl ? 0 : (size_t)a.gbdt_trees * L * sizeof(float);
  if (gl) {
    if (a.rules) hipLaunchKernelGGL((score_gbdt_g32_kernel<D, R, true, true, kG20>), dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((score_gbdt_g32_kernel<D, R, false, true, kG20>), dim3(grid), dim3(256), 0, s, a);
  } else {
    if (a.rules) hipLaunchKernelGGL((score_gbdt_g32_kernel<D, R, true, false, kG20>), dim3(grid), dim3(256), lds, s, a);
    else hipLaunchKernelGGL((score_gbdt_g32_kernel<D, R, false, false, kG20>), dim3(grid), dim3(256), lds, s, a);
  }
}

template <int D>
static void launch_g32_d(const ccfd_score_args& a, hipStream_t s) {
  if (a.flags & CCFD_ARG_WIRE_G20) {             // G20: one chunk per wave step
    launch_g32_r<D, 1, true>(a, s);
    return;
  }
  const int r = g32_env("CCFD_G32_R", 1, 1, 2);
  if (r == 2) launch_g32_r<D, 2, false>(a, s);
  else launch_g32_r<D, 1, false>(a, s);
}

int launch_gbdt_g32(const ccfd_score_args& a, hipStream_t s) {
  if (a.gbdt_trees <= 0 || a.gbdt_depth < 1 || a.gbdt_depth > 8) return -2;
  if (a.n <= 0) return 0;
  dispatch_depth(a.gbdt_depth, [&](auto d) { launch_g32_d<decltype(d)::value>(a, s); });
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace ccfd

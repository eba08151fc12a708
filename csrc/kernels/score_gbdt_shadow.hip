// Shadow scoring for oblivious GBDTs on G32 / G20 rows: a challenger ensemble scored beside
// the champion on the same binned rows in the same pass.
//
// A 64-row chunk is fetched, transposed and lifted into 30 VGPRs ONCE (g32_core.h: gx_fetch,
// gx_rows, gx_lift); the tree walk then runs twice over those registers, first with the
// champion's split parameters and leaf table, then with the challenger's.  Both walks are the
// same g32_trees<D, 1> code, so a model's leaf sum is formed in the same order whether it
// rides as champion or as shadow: B scored as A's shadow carries the bits of B scored alone.
//
//   * score_gbdt_shadow_kernel: one launch per micro-batch, the counterpart of
//     score_gbdt_g32_kernel (R = 1).
//   * persist_gbdt_shadow_kernel: the claimed-item path of persist_gbdt_g32_kernel with its
//     one-chunk prefetch ring; doorbell workgroup, claim, item completion and flag list are
//     those of persist_core.h, unchanged.
//
// The champion's epilogue is what the champion kernels do (g32_core.h g32_row_epilogue: proba,
// route, amount histogram, counters; then flag list and completion record).  The challenger
// adds the five CCFD_CNT_SHADOW_* counters (shadow_core.h) and, in the launch kernel, its
// proba_1 per row when asked to.  Stale rows (bin stamp != the champion blob's) are counted in
// no shadow slot.
//
// The challenger has the champion's shape (T trees x depth D) and bin table: the host side
// checks that, the kernels trust it.  Leaf tables: the champion's placement follows its own
// kernel's rule; the challenger's table is staged behind it in the same dynamic-LDS
// allocation while both fit kG32LeafLds floats, else gathered from its blob (kGS).  Threshold
// route only.
#include "g32_core.h"
#include "persist_core.h"
#include "shadow_core.h"

namespace ccfd {

namespace {

// LDS offset (floats) of the challenger's leaf table behind the champion's: 16-byte aligned
// for the float4 staging copy (T * 2^D is odd or 2 mod 4 only at depth 1).
__host__ __device__ constexpr int shadow_leaf_off(int T, int D) { return ((T << D) + 3) & ~3; }

// Champion A and challenger B of a kernel, leaf tables placed (kGL / kGS: the champion's /
// the challenger's leaves from global memory; kGL implies kGS); the caller's barrier follows.
struct ShadowPair {
  G32Model A, B;
  const float *leavesA, *leavesB;
  int T;
};

template <int D, bool kGL, bool kGS>
__device__ __forceinline__ ShadowPair shadow_pair(const void* blobA, const void* blobB, int T, float* lv, int tid) {
  ShadowPair m{g32_model<D>(blobA, T), g32_model<D>(blobB, T), nullptr, nullptr, T};
  m.leavesA = g32_leaves<D, kGL>(m.A, T, lv, tid, 256);
  m.leavesB = g32_leaves<D, kGS>(m.B, T, lv + shadow_leaf_off(T, D), tid, 256);
  return m;
}

// This wave's counts: the champion's, the challenger's, and the fresh rows both scored.
struct ShadowWave {
  G32Wave w;
  ShadowAcc sw;
  unsigned srows = 0;
};

// One fetched 64-row chunk through both ensembles: transpose, lift, two tree walks, the
// champion's row epilogue and the challenger's bookkeeping.  Returns the champion's row for
// the caller's flag list.  `b0`: the 30 registers the bins are lifted into, declared in the
// caller's loop body (declared here, the persistent kernel needs 6 more VGPRs and loses a wave
// per SIMD at depths 4..6).
template <int D, bool kG20>
__device__ __forceinline__ G32RowOut shadow_chunk(const ShadowPair& m, uint4* xt, G32Row& cur, unsigned (&b0)[kF],
                                                  int lane, int row, int n, float thr, EpilogueLds& epi, ShadowWave& s,
                                                  float* proba, uint8_t* route, float* shadow_proba) {
  gx_rows<kG20>(xt, lane, cur);
  const unsigned meta = gx_lift<kG20>(cur, b0);                // bucket | stamp << 8
  float accA[1], accB[1];
  g32_trees<D, 1>(b0, b0, m.leavesA, m.A.feat, m.A.kbin, m.T, accA);
  g32_trees<D, 1>(b0, b0, m.leavesB, m.B.feat, m.B.kbin, m.T, accB);
  const G32RowOut o = g32_row_epilogue<false>(epi, s.w, m.A, meta, accA[0], row, n, thr, nullptr, proba, route);
  const bool scored = o.valid && o.fresh;
  const float q = o.fresh ? sigmoid(m.B.base + accB[0]) : __builtin_nanf("");
  const bool sf = scored && (q >= thr);
  if (o.valid && shadow_proba) st_g(shadow_proba + row, q);
  if (scored) shadow_row(s.sw, o.p, q);
  s.srows += __popcll(__ballot(scored));
  s.sw.fraud += __popcll(__ballot(sf));
  s.sw.both += __popcll(__ballot(sf && o.fr));
  return o;
}

// ---------------------------------------------------------------------------------------
// Launch kernel.
// ---------------------------------------------------------------------------------------
template <int D, bool kGL, bool kGS, bool kG20>
__global__ __launch_bounds__(256) void score_gbdt_shadow_kernel(ccfd_shadow_args sa) {
  extern __shared__ __attribute__((aligned(16))) float lv[];   // champion's, then challenger's leaves
  __shared__ uint4 xt[kG32Waves][128];                         // per-wave chunk transpose
  __shared__ EpilogueLds epi;
  __shared__ ShadowLds sh;
  const ccfd_score_args& a = sa.base;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = a.n;
  const int nchunks = (n + kG32Rows - 1) / kG32Rows;
  const int gstride = gridDim.x * kG32Waves;
  int chunk = blockIdx.x * kG32Waves + wave;
  const unsigned char* __restrict__ xb = reinterpret_cast<const unsigned char*>(a.x);

  // rows first: the host-memory latency overlaps the leaf staging below
  G32Row pre;
  gx_fetch<kG20>(xb, n, chunk, lane, pre);

  epi_init(epi);
  shadow_init(sh);
  stamp_start(a, blockIdx.x);
  const ShadowPair m = shadow_pair<D, kGL, kGS>(a.blob, sa.shadow_blob, a.gbdt_trees, lv, tid);
  __syncthreads();                                              // leaves staged, epi / sh initialised

  const float thr = a.threshold;
  ShadowWave s;
  for (; chunk < nchunks; chunk += gstride) {
    G32Row cur = pre;
    const int nxt = chunk + gstride;
    if (nxt < nchunks) gx_fetch<kG20>(xb, n, nxt, lane, pre);
    unsigned b0[kF];
    const int row = chunk * kG32Rows + lane;
    const G32RowOut o = shadow_chunk<D, kG20>(m, xt[wave], cur, b0, lane, row, n, thr, epi, s, a.proba, a.route,
                                              sa.shadow_proba);
    emit_flagged(a, o.fr, row);
  }
  g32_wave_commit(epi, s.w, a.counters, lane);
  shadow_wave_commit(sh, s.sw, s.srows, lane);
  epi_flush(epi, a.counters);                                   // barrier first, then the champion's atomics
  if (tid == 2 * kNB + 1) shadow_flush(sh, a.counters);
  signal_done(a, gridDim.x);
}

// ---------------------------------------------------------------------------------------
// Persistent kernel: claimed items of 4 waves x `cpw` 64-row chunks, the next chunk of a wave
// in flight while the current one goes through both ensembles.
// ---------------------------------------------------------------------------------------
template <int D, bool kGL, bool kGS, bool kG20>
__global__ __launch_bounds__(256) void persist_gbdt_shadow_kernel(ccfd_persist_shadow_args sa) {
  extern __shared__ __attribute__((aligned(16))) float lv[];   // champion's, then challenger's leaves
  __shared__ uint4 xt[kG32Waves][128];
  __shared__ EpilogueLds epi;
  __shared__ ShadowLds sh;
  __shared__ ccfd_persist_desc sdesc;
  __shared__ unsigned long long s_item;
  __shared__ int s_cmd;
  const ccfd_persist_args& a = sa.base;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int C = a.items_per_batch;
  const int cpw = a.tiles_per_wave;                       // 64-row chunks per wave per item
  if (blockIdx.x == 0) {                                  // doorbell (persist_core.h)
    if (wave == 0) persist_doorbell(a, lane);
    return;                                               // no barrier is ever used by WG 0
  }
  const ShadowPair m = shadow_pair<D, kGL, kGS>(a.blob, sa.shadow_blob, a.gbdt_trees, lv, tid);
  epi_init(epi);
  shadow_init(sh);
  __syncthreads();
  unsigned long long posted_cache = 0;                    // thread 0 only
  const float thr = a.threshold;

  for (;;) {
    if (tid == 0) persist_claim(a, C, posted_cache, sdesc, s_item, s_cmd);
    __syncthreads();
    if (s_cmd) break;
    const ccfd_persist_desc d = sdesc;                     // registers: no LDS wait in the epilogue
    const PersistItem it = persist_item(a, d, s_item, C, kG32Waves * cpw, wave, tid == 0);   // K7: item 0 is claimed first
    const int n = it.n;

    ShadowWave s;                                          // this wave's share of the item
    G32Row pre;
    if (it.u0 * kG32Rows < n) gx_fetch<kG20>(it.xb, n, it.u0, lane, pre);
#pragma unroll 1
    for (int k = 0; k < cpw; ++k) {
      const int chunk = it.u0 + kG32Waves * k;             // this wave's chunks: u0 + 4k
      if (chunk * kG32Rows >= n) break;                    // wave-uniform
      G32Row cur = pre;
      if (k + 1 < cpw && (chunk + kG32Waves) * kG32Rows < n) gx_fetch<kG20>(it.xb, n, chunk + kG32Waves, lane, pre);
      unsigned b0[kF];
      const int row = chunk * kG32Rows + lane;
      const G32RowOut o = shadow_chunk<D, kG20>(m, xt[wave], cur, b0, lane, row, n, thr, epi, s, d.proba, d.route,
                                                nullptr);
      persist_emit_flagged(a, d, it.slot, o.m, o.fr, row, lane);
    }
    unsigned long long* cnt = a.counters[d.epoch & 1];
    g32_item_commit(epi, s.w, cnt, lane);
    shadow_wave_commit(sh, s.sw, s.srows, lane);
    // the item's challenger counters, then LDS reset for the next item: persist_item_done's
    // barriers and its vmcnt(0) drain order both before the item's ticket and the next claim
    __syncthreads();
    if (tid == 96) {
      shadow_flush(sh, cnt);
      sh.rows = 0; sh.fraud = 0; sh.both = 0; sh.psum_e6 = 0; sh.absdiff_e6 = 0;
    }
    persist_item_done(a, epi, d, it.slot, C, tid);
  }
}

// Leaf placement of a pair: the champion's own rule (`gl`), the challenger's table behind the
// champion's while both fit kG32LeafLds floats.
struct ShadowLeafPlan {
  bool gl, gs;
  size_t lds;
};

ShadowLeafPlan shadow_leaf_plan(int T, int D, long champion_lds_max) {
  const long nl = (long)T << D;
  ShadowLeafPlan p;
  p.gl = nl > champion_lds_max || g32_env("CCFD_G32_GLOBAL_LEAVES", 0, 0, 1);
  p.gs = p.gl || (long)shadow_leaf_off(T, D) + nl > kG32LeafLds;
  p.lds = p.gl ? 0 : (p.gs ? (size_t)nl : (size_t)shadow_leaf_off(T, D) + (size_t)nl) * sizeof(float);
  return p;
}

// Grid as launch_g32_r (score_gbdt_g32.hip) at R = 1: one wave per chunk, capped at
// CCFD_G32_WGS_PER_CU workgroups per CU; a launch keeps the champion's leaves in LDS up to
// 32 KB (its rule there), which leaves room for the challenger's.
template <int D, bool kG20>
void launch_shadow_f(const ccfd_shadow_args& sa, hipStream_t s) {
  const ccfd_score_args& a = sa.base;
  const int wgs_per_cu = g32_env("CCFD_G32_WGS_PER_CU", 4, 1, 8);   // read per launch: sweepable in-process
  const int nchunks = (a.n + kG32Rows - 1) / kG32Rows;
  int grid = (nchunks + kG32Waves - 1) / kG32Waves;
  const int cap = 256 * wgs_per_cu;
  grid = grid < 1 ? 1 : (grid > cap ? cap : grid);
  const ShadowLeafPlan p = shadow_leaf_plan(a.gbdt_trees, D, kG32LeafLds / 2);
  // two tables of <= 32 KB always fit: both in LDS or both in global memory
  if (p.gl || p.gs) hipLaunchKernelGGL((score_gbdt_shadow_kernel<D, true, true, kG20>), dim3(grid), dim3(256), 0, s, sa);
  else hipLaunchKernelGGL((score_gbdt_shadow_kernel<D, false, false, kG20>), dim3(grid), dim3(256), p.lds, s, sa);
}

template <int D, bool kG20>
int launch_persist_shadow_f(const ccfd_persist_shadow_args& sa, int grid, hipStream_t s) {
  const ShadowLeafPlan p = shadow_leaf_plan(sa.base.gbdt_trees, D, kG32LeafLds);
  if (p.gl) hipLaunchKernelGGL((persist_gbdt_shadow_kernel<D, true, true, kG20>), dim3(grid), dim3(256), 0, s, sa);
  else if (p.gs) hipLaunchKernelGGL((persist_gbdt_shadow_kernel<D, false, true, kG20>), dim3(grid), dim3(256), p.lds, s, sa);
  else hipLaunchKernelGGL((persist_gbdt_shadow_kernel<D, false, false, kG20>), dim3(grid), dim3(256), p.lds, s, sa);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace

int launch_gbdt_shadow(const ccfd_shadow_args& sa, hipStream_t s) {
  const ccfd_score_args& a = sa.base;
  if (a.gbdt_trees <= 0 || a.gbdt_depth < 1 || a.gbdt_depth > 8) return -2;
  if (a.n <= 0) return 0;
  dispatch_depth(a.gbdt_depth, [&](auto d) {
    if (a.flags & CCFD_ARG_WIRE_G20) launch_shadow_f<decltype(d)::value, true>(sa, s);
    else launch_shadow_f<decltype(d)::value, false>(sa, s);
  });
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int launch_persist_gbdt_shadow(const ccfd_persist_shadow_args& sa, int grid, hipStream_t s) {
  const ccfd_persist_args& a = sa.base;
  if (a.gbdt_trees <= 0 || a.gbdt_depth < 1 || a.gbdt_depth > 8) return -2;
  return dispatch_depth(a.gbdt_depth, [&](auto d) {
    return (a.flags & CCFD_ARG_WIRE_G20) ? launch_persist_shadow_f<decltype(d)::value, true>(sa, grid, s)
                                         : launch_persist_shadow_f<decltype(d)::value, false>(sa, grid, s);
  });
}

}  // namespace ccfd

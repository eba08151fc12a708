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
// The champion's epilogue is what the champion kernels do (proba, route, flag list, amount
// histogram, counters, completion record).  The challenger adds the five CCFD_CNT_SHADOW_*
// counters (shadow_core.h) and, in the launch kernel, its proba_1 per row when asked to.
// Stale rows (bin stamp != the champion blob's) are counted in no shadow slot.
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

// Split parameters and leaf table of one GBB1 blob.
struct G32Model {
  g32_cint_p feat, kbin;
  float base;
};

template <int D>
__device__ __forceinline__ G32Model g32_model(const char* blob, int T) {
  const int tdw = ((4 * T * D + 15) & ~15) / 4;
  // CONSTANT address space: wave-uniform indices compile to scalar loads (g32_core.h)
  return G32Model{(g32_cint_p)(blob + kHeader), (g32_cint_p)(blob + kHeader + 4 * tdw),
                  *reinterpret_cast<const float*>(blob + 16)};
}

// LDS offset (floats) of the challenger's leaf table behind the champion's: 16-byte aligned
// for the float4 staging copy (T * 2^D is odd or 2 mod 4 only at depth 1).
__host__ __device__ constexpr int shadow_leaf_off(int T, int D) { return ((T << D) + 3) & ~3; }

// ---------------------------------------------------------------------------------------
// Launch kernel.  kGL: champion leaves from global memory; kGS: challenger leaves from
// global memory (kGL implies kGS).
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
  const char* blobA = reinterpret_cast<const char*>(a.blob);
  const char* blobB = reinterpret_cast<const char*>(sa.shadow_blob);
  const int T = a.gbdt_trees;
  const unsigned stamp = (unsigned)*reinterpret_cast<const int*>(blobA + 20);
  const G32Model A = g32_model<D>(blobA, T), B = g32_model<D>(blobB, T);
  const float* leavesA = lv;
  const float* leavesB = lv + shadow_leaf_off(T, D);
  if constexpr (kGL) leavesA = g32_leaves_global(blobA, T, D);
  else g32_stage_leaves<D>(blobA, T, lv, tid, 256);
  if constexpr (kGS) leavesB = g32_leaves_global(blobB, T, D);
  else g32_stage_leaves<D>(blobB, T, lv + shadow_leaf_off(T, D), tid, 256);
  __syncthreads();                                              // leaves staged, epi / sh initialised

  const float thr = a.threshold;
  unsigned fraud = 0, rows = 0, stale = 0, srows = 0;
  unsigned long long psum = 0;
  ShadowAcc sw;
  for (; chunk < nchunks; chunk += gstride) {
    unsigned b0[kF];
    G32Row cur = pre;
    gx_rows<kG20>(xt[wave], lane, cur);
    const unsigned meta = gx_lift<kG20>(cur, b0);              // bucket | stamp << 8
    const int nxt = chunk + gstride;
    if (nxt < nchunks) gx_fetch<kG20>(xb, n, nxt, lane, pre);
    float accA[1], accB[1];
    g32_trees<D, 1>(b0, b0, leavesA, A.feat, A.kbin, T, accA);
    g32_trees<D, 1>(b0, b0, leavesB, B.feat, B.kbin, T, accB);
    const int row = chunk * kG32Rows + lane;
    const bool valid = row < n;
    const bool fresh = ((meta >> 8) & 0xffu) == stamp;
    const float p = fresh ? sigmoid(A.base + accA[0]) : __builtin_nanf("");
    const float q = fresh ? sigmoid(B.base + accB[0]) : __builtin_nanf("");
    const bool fr = valid && fresh && (p >= thr);
    const bool sf = valid && fresh && (q >= thr);
    if (valid) {
      if (a.proba) st_g(a.proba + row, p);
      if (a.route) st_g(a.route + row, (uint8_t)(fr ? 1 : 0));
      if (sa.shadow_proba) st_g(sa.shadow_proba + row, q);
      if (fresh) {
        psum += (unsigned)(p * 1e6f + 0.5f);
        shadow_row(sw, p, q);
      }
      atomicAdd(&epi.hist[(fr ? kNB : 0) + min((int)(meta & 0xffu), kNB - 1)], 1u);
    }
    fraud += __popcll(__ballot(fr));
    rows += __popcll(__ballot(valid));
    stale += __popcll(__ballot(valid && !fresh));
    srows += __popcll(__ballot(valid && fresh));
    sw.fraud += __popcll(__ballot(sf));
    sw.both += __popcll(__ballot(sf && fr));
    emit_flagged(a, fr, row);
  }
  psum = wave_sum_u64(psum);
  if (lane == 0) {
    atomicAdd(&epi.fraud, fraud);
    atomicAdd(&epi.rows, rows);
    atomicAdd(&epi.psum_e6, psum);
  }
  shadow_wave_commit(sh, sw, srows, lane);
  unsigned long long* cnt = a.counters;
  if (cnt != nullptr && lane == 0 && stale) atomicAdd(&cnt[CCFD_CNT_WIRE_STALE], (unsigned long long)stale);
  epi_flush(epi, cnt);                                          // barrier first, then the champion's atomics
  if (tid == 2 * kNB + 1) shadow_flush(sh, cnt);
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
  const char* blobA = reinterpret_cast<const char*>(a.blob);
  const char* blobB = reinterpret_cast<const char*>(sa.shadow_blob);
  const int T = a.gbdt_trees;
  const unsigned stamp = (unsigned)*reinterpret_cast<const int*>(blobA + 20);
  const G32Model A = g32_model<D>(blobA, T), B = g32_model<D>(blobB, T);
  const float* leavesA = lv;
  const float* leavesB = lv + shadow_leaf_off(T, D);
  if constexpr (kGL) leavesA = g32_leaves_global(blobA, T, D);
  else g32_stage_leaves<D>(blobA, T, lv, tid, 256);
  if constexpr (kGS) leavesB = g32_leaves_global(blobB, T, D);
  else g32_stage_leaves<D>(blobB, T, lv + shadow_leaf_off(T, D), tid, 256);
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
    const int item = (int)(s_item % (unsigned long long)C);
    const int slot = (int)(d.seq % (unsigned long long)a.ring);
    const int n = d.n;
    const unsigned char* xb = reinterpret_cast<const unsigned char*>(d.x);
    if (item == 0 && tid == 0)                             // K7: micro-batch start (item 0 claimed first)
      __hip_atomic_store(&a.dev->tstart[slot], wall_clock64(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int c0 = item * (kG32Waves * cpw) + wave;        // this wave's chunks: c0 + 4k

    unsigned fraud = 0, rows = 0, stale = 0, srows = 0;    // this wave's share of the item
    unsigned long long psum = 0;
    ShadowAcc sw;
    G32Row pre;
    if (c0 * kG32Rows < n) gx_fetch<kG20>(xb, n, c0, lane, pre);
#pragma unroll 1
    for (int k = 0; k < cpw; ++k) {
      const int chunk = c0 + kG32Waves * k;
      if (chunk * kG32Rows >= n) break;                    // wave-uniform
      G32Row cur = pre;
      if (k + 1 < cpw && (chunk + kG32Waves) * kG32Rows < n) gx_fetch<kG20>(xb, n, chunk + kG32Waves, lane, pre);
      gx_rows<kG20>(xt[wave], lane, cur);
      unsigned b0[kF];
      const unsigned meta = gx_lift<kG20>(cur, b0);
      float accA[1], accB[1];
      g32_trees<D, 1>(b0, b0, leavesA, A.feat, A.kbin, T, accA);
      g32_trees<D, 1>(b0, b0, leavesB, B.feat, B.kbin, T, accB);
      const int row = chunk * kG32Rows + lane;
      const bool valid = row < n;
      const bool fresh = ((meta >> 8) & 0xffu) == stamp;
      const float p = fresh ? sigmoid(A.base + accA[0]) : __builtin_nanf("");
      const float q = fresh ? sigmoid(B.base + accB[0]) : __builtin_nanf("");
      const bool fr = valid && fresh && (p >= thr);
      const bool sf = valid && fresh && (q >= thr);
      if (valid) {
        if (d.proba) st_g(d.proba + row, p);
        if (d.route) st_g(d.route + row, (uint8_t)(fr ? 1 : 0));
        if (fresh) {
          psum += (unsigned)(p * 1e6f + 0.5f);
          shadow_row(sw, p, q);
        }
        atomicAdd(&epi.hist[(fr ? kNB : 0) + min((int)(meta & 0xffu), kNB - 1)], 1u);
      }
      const unsigned long long m = __ballot(fr);
      fraud += __popcll(m);
      rows += __popcll(__ballot(valid));
      stale += __popcll(__ballot(valid && !fresh));
      srows += __popcll(__ballot(valid && fresh));
      sw.fraud += __popcll(__ballot(sf));
      sw.both += __popcll(__ballot(sf && fr));
      persist_emit_flagged(a, d, slot, m, fr, row, lane);
    }
    psum = wave_sum_u64(psum);
    unsigned long long* cnt = a.counters[d.epoch & 1];
    if (lane == 0 && rows) {
      atomicAdd(&epi.fraud, fraud);
      atomicAdd(&epi.rows, rows);
      atomicAdd(&epi.psum_e6, psum);
      if (stale && cnt) atomicAdd(&cnt[CCFD_CNT_WIRE_STALE], (unsigned long long)stale);
    }
    shadow_wave_commit(sh, sw, srows, lane);
    // the item's challenger counters, then LDS reset for the next item: persist_item_done's
    // barriers and its vmcnt(0) drain order both before the item's ticket and the next claim
    __syncthreads();
    if (tid == 96) {
      shadow_flush(sh, cnt);
      sh.rows = 0; sh.fraud = 0; sh.both = 0; sh.psum_e6 = 0; sh.absdiff_e6 = 0;
    }
    persist_item_done(a, epi, d, slot, C, tid);
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

template <int D>
void launch_shadow_d(const ccfd_shadow_args& sa, hipStream_t s) {
  if (sa.base.flags & CCFD_ARG_WIRE_G20) launch_shadow_f<D, true>(sa, s);
  else launch_shadow_f<D, false>(sa, s);
}

template <int D, bool kG20>
int launch_persist_shadow_f(const ccfd_persist_shadow_args& sa, int grid, hipStream_t s) {
  const ShadowLeafPlan p = shadow_leaf_plan(sa.base.gbdt_trees, D, kG32LeafLds);
  if (p.gl) hipLaunchKernelGGL((persist_gbdt_shadow_kernel<D, true, true, kG20>), dim3(grid), dim3(256), 0, s, sa);
  else if (p.gs) hipLaunchKernelGGL((persist_gbdt_shadow_kernel<D, false, true, kG20>), dim3(grid), dim3(256), p.lds, s, sa);
  else hipLaunchKernelGGL((persist_gbdt_shadow_kernel<D, false, false, kG20>), dim3(grid), dim3(256), p.lds, s, sa);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

template <int D>
int launch_persist_shadow_d(const ccfd_persist_shadow_args& sa, int grid, hipStream_t s) {
  return (sa.base.flags & CCFD_ARG_WIRE_G20) ? launch_persist_shadow_f<D, true>(sa, grid, s)
                                             : launch_persist_shadow_f<D, false>(sa, grid, s);
}

}  // namespace

int launch_gbdt_shadow(const ccfd_shadow_args& sa, hipStream_t s) {
  const ccfd_score_args& a = sa.base;
  if (a.gbdt_trees <= 0 || a.gbdt_depth < 1 || a.gbdt_depth > 8) return -2;
  if (a.n <= 0) return 0;
  switch (a.gbdt_depth) {
    case 1: launch_shadow_d<1>(sa, s); break;
    case 2: launch_shadow_d<2>(sa, s); break;
    case 3: launch_shadow_d<3>(sa, s); break;
    case 4: launch_shadow_d<4>(sa, s); break;
    case 5: launch_shadow_d<5>(sa, s); break;
    case 6: launch_shadow_d<6>(sa, s); break;
    case 7: launch_shadow_d<7>(sa, s); break;
    default: launch_shadow_d<8>(sa, s); break;
  }
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int launch_persist_gbdt_shadow(const ccfd_persist_shadow_args& sa, int grid, hipStream_t s) {
  const ccfd_persist_args& a = sa.base;
  if (a.gbdt_trees <= 0 || a.gbdt_depth < 1 || a.gbdt_depth > 8) return -2;
  switch (a.gbdt_depth) {
    case 1: return launch_persist_shadow_d<1>(sa, grid, s);
    case 2: return launch_persist_shadow_d<2>(sa, grid, s);
    case 3: return launch_persist_shadow_d<3>(sa, grid, s);
    case 4: return launch_persist_shadow_d<4>(sa, grid, s);
    case 5: return launch_persist_shadow_d<5>(sa, grid, s);
    case 6: return launch_persist_shadow_d<6>(sa, grid, s);
    case 7: return launch_persist_shadow_d<7>(sa, grid, s);
    default: return launch_persist_shadow_d<8>(sa, grid, s);
  }
}

}  // namespace ccfd

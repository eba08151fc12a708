// General (non-oblivious) tree ensembles on binned rows: G32 (32 B) and G20 (20 B) rows against
// an 'FRB1' blob (models/forest.py) -- the node table of score_forest.hip with a node's
// threshold replaced by its bin index k, so a step asks `bin[feat] > k`, which is exactly the
// f32 `x[feat] > thr` (g32_core.h).  One launch per micro-batch.
//
// Layout per 256-thread workgroup (the oblivious G32 structure, g32_core.h):
//   * a wave owns 64-row chunks, one row per lane, and strides over them on the grid; a chunk
//     is fetched with full-width wave loads, transposed through the wave's LDS tile and lifted
//     (gx_fetch / gx_rows / gx_lift), with the next chunk in flight while this one is walked;
//     no workgroup barrier inside the chunk loop;
//   * a general tree's feature id differs per lane, so the bins cannot stay in VGPRs (a
//     register index must be wave-uniform): each lane writes its 30 bins back into the same
//     tile, four a dword, DWORD-MAJOR (tile[w][lane], w < 8).  A step reads tile[feat >> 2][lane]
//     -- bank `lane mod 32` for ANY per-lane feat, conflict-free within each 32-lane group of a
//     ds_read_b32 -- and extracts byte `feat & 3`.  G20 rows are re-packed to the same byte form,
//     so both formats share one walk;
//   * the node table is staged once per workgroup in LDS when it fits kNodeLdsBytes, otherwise
//     walked from global memory (L2), as in score_forest.hip; a lane walks several trees at once;
//   * the scored row goes through the binned kernels' epilogue (g32_row_epilogue: stale stamp
//     -> NaN + CCFD_CNT_WIRE_STALE, amount bucket from the row, proba-only rules) with the
//     blob's link applied here.
//
// All LDS is one dynamic region -- [wave tiles][epilogue][node table] -- so the node table's
// 8- and 16-byte accesses are aligned whatever the compiler does with static LDS.
#include <cstring>
#include <string>

#include "forest_core.h"
#include "g32_core.h"

namespace ccfd {

void set_error(const std::string& e);

// Independent tree walks per lane, as in score_forest.hip: compile-time knobs of their own,
// because a step here has a byte extract the f32 step lacks.  Measured on 16 M HBM-resident G32
// rows (profiles/forest/walk_ilp_ab_bins.jsonl).  LDS table (100 complete depth-6 trees) --
// 4: 2.06, 8: 2.45, 16: 2.63, 32: 2.70 G rows/s; 16 keeps the kernel at 103..115 VGPRs, i.e. the
// 4 waves per SIMD that four workgroups of a small table need.  Global table (256 random
// depth-12 trees) -- 1: 0.58, 2: 0.40, 4: 0.41 G rows/s.
#ifndef CCFD_FOREST_BINS_ILP_LDS
#define CCFD_FOREST_BINS_ILP_LDS 16
#endif
#ifndef CCFD_FOREST_BINS_ILP_GLOBAL
#define CCFD_FOREST_BINS_ILP_GLOBAL 1
#endif
constexpr int kFbIlpLds = CCFD_FOREST_BINS_ILP_LDS;
constexpr int kFbIlpGlobal = CCFD_FOREST_BINS_ILP_GLOBAL;

constexpr int kFbTileBytes = kG32Waves * 128 * (int)sizeof(uint4);                      // 4 x 2 KB
constexpr int kFbFixedLds = kFbTileBytes + (((int)sizeof(EpilogueLds) + 15) & ~15);      // node table starts here
static_assert(kFbFixedLds % 16 == 0 && kFbFixedLds + kNodeLdsBytes <= 160 * 1024, "one workgroup's LDS");

// The lane's 30 bins, four a dword, into column `col` (= tile + lane) of the wave's tile.  Only
// this lane reads the column back, so no barrier follows.
__device__ __forceinline__ void fb_store_bins(unsigned* col, const unsigned (&b)[kF]) {
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    unsigned v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * w + j < kF) v |= b[4 * w + j] << (8 * j);
    col[w * kG32Rows] = v;
  }
}

// Walk trees t0 .. t0 + U - 1 for the lane's row; returns the leaf sum.  The branch-free step
// of fr_walk (score_forest.hip): a leaf's child field is its own index and its feature field
// is 0, so a finished lane stays put and its (ignored) bin read is in bounds.  `(w & 0x1c) << 4`
// is dword (feat >> 2) * 64 of the column, at most 7 * 64 + 63 of the tile's 512.
template <int U, bool kLds>
__device__ __forceinline__ float fb_walk(const int* __restrict__ tree, const uint2* __restrict__ gn, const uint2* ln,
                                         const unsigned* col, int t0) {
  FrNode nd[U];
  int depth = 0;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int t = t0 + u;
    const unsigned root = (unsigned)__builtin_amdgcn_readfirstlane(tree[2 * t]);
    depth = max(depth, __builtin_amdgcn_readfirstlane(tree[2 * t + 1]));
    nd[u] = fr_node<kLds>(gn, ln, root);
  }
  for (int s = 0; s < depth; ++s) {
    unsigned x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) x[u] = col[(nd[u].w & 0x1cu) << 4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned inner = ((nd[u].w >> 5) & 1u) ^ 1u;
      const unsigned bin = (x[u] >> ((nd[u].w & 3u) * 8u)) & 0xffu;
      const unsigned gt = bin > __float_as_uint(nd[u].v) ? 1u : 0u;
      nd[u] = fr_node<kLds>(gn, ln, (nd[u].w >> 8) + (gt & inner));
    }
  }
  float acc = 0.f;
#pragma unroll
  for (int u = 0; u < U; ++u) acc += nd[u].v;
  return acc;
}

// The trees, kU at a time, then the tail in halving group sizes.
template <int U, bool kLds>
__device__ __forceinline__ void fb_tail(const int* __restrict__ tree, const uint2* __restrict__ gn, const uint2* ln,
                                        const unsigned* col, int T, int& t, float& acc) {
  if (t + U <= T) { acc += fb_walk<U, kLds>(tree, gn, ln, col, t); t += U; }
  if constexpr (U > 1) fb_tail<U / 2, kLds>(tree, gn, ln, col, T, t, acc);
}

template <bool kLds>
__device__ __forceinline__ float fb_sum(const int* __restrict__ tree, const uint2* __restrict__ gn, const uint2* ln,
                                        const unsigned* col, int T) {
  constexpr int kU = kLds ? kFbIlpLds : kFbIlpGlobal;
  static_assert((kU & (kU - 1)) == 0, "group sizes halve down to 1");
  float acc = 0.f;
  int t = 0;
  for (; t + kU <= T; t += kU) acc += fb_walk<kU, kLds>(tree, gn, ln, col, t);
  if constexpr (kU > 1) fb_tail<kU / 2, kLds>(tree, gn, ln, col, T, t, acc);
  return acc;
}

// The node table into LDS, by the whole workgroup.  16-byte copies: the node section is padded
// to 16 B, and so is its LDS.  Eight loads are in flight per thread before the first store,
// where a load-wait-store loop pays one L2 round trip per 4 KB of table; a 65536-row micro-batch
// is one chunk per wave, so the staging is a visible part of its launch.
__device__ __forceinline__ void fb_stage_nodes(const uint2* __restrict__ gn, uint2* nl, int n_nodes, int tid) {
  constexpr int kInFlight = 8;
  const uint4* s4 = reinterpret_cast<const uint4*>(gn);
  uint4* d4 = reinterpret_cast<uint4*>(nl);
  const int n16 = (n_nodes + 1) / 2;
  for (int i0 = tid; i0 < n16; i0 += 256 * kInFlight) {
    uint4 v[kInFlight];
#pragma unroll
    for (int k = 0; k < kInFlight; ++k)
      if (i0 + 256 * k < n16) v[k] = ld_g16(s4 + i0 + 256 * k);
#pragma unroll
    for (int k = 0; k < kInFlight; ++k)
      if (i0 + 256 * k < n16) d4[i0 + 256 * k] = v[k];
  }
}

// `lds_nodes`: nodes the launch allocated LDS for (0 = none).  T, n_nodes, the link and the
// stamp come from the blob's own header, so what bounds every read is the blob itself.
template <bool kR, bool kG20>
__global__ __launch_bounds__(256) void score_forest_bins_kernel(ccfd_score_args a, int lds_nodes) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fb_lds[];
  uint4* xt = reinterpret_cast<uint4*>(fb_lds);                                 // [kG32Waves][128]
  EpilogueLds& epi = *reinterpret_cast<EpilogueLds*>(fb_lds + kFbTileBytes);
  uint2* nl = reinterpret_cast<uint2*>(fb_lds + kFbFixedLds);                   // lds_nodes nodes

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = a.n;
  const int nchunks = (n + kG32Rows - 1) / kG32Rows;
  const int stride = gridDim.x * kG32Waves;
  int c = blockIdx.x * kG32Waves + wave;
  const unsigned char* __restrict__ xb = reinterpret_cast<const unsigned char*>(a.x);

  // rows first: their latency overlaps the node staging below (a chunk past the batch is
  // clamped into it by the fetch and never scored)
  G32Row pre;
  gx_fetch<kG20>(xb, n, c, lane, pre);

  epi_init(epi);
  stamp_start(a, blockIdx.x);

  const char* blob = reinterpret_cast<const char*>(a.blob);
  const int* __restrict__ hdr = reinterpret_cast<const int*>(blob);
  const bool sig = (hdr[1] & 1) != 0;
  const int T = hdr[2];
  const int n_nodes = hdr[5];
  const G32Model M{nullptr, nullptr, nullptr, gbb_base(blob), (unsigned)hdr[6]};
  const int* __restrict__ tree = reinterpret_cast<const int*>(blob + kHeader);
  const uint2* __restrict__ gn = reinterpret_cast<const uint2*>(blob + kHeader + ((8 * (size_t)T + 15) & ~(size_t)15));
  const bool resident = n_nodes <= lds_nodes;
  if (resident) fb_stage_nodes(gn, nl, n_nodes, tid);
  __syncthreads();                                              // nodes staged, epi initialised

  uint4* tile = xt + wave * 128;
  unsigned* col = reinterpret_cast<unsigned*>(tile) + lane;
  G32Wave w;
  for (; c < nchunks; c += stride) {
    G32Row cur = pre;
    gx_rows<kG20>(tile, lane, cur);
    unsigned b[kF];
    const unsigned meta = gx_lift<kG20>(cur, b);                // bucket | stamp << 8
    fb_store_bins(col, b);
    if (c + stride < nchunks) gx_fetch<kG20>(xb, n, c + stride, lane, pre);

    const float z = M.base + (resident ? fb_sum<true>(tree, gn, nl, col, T) : fb_sum<false>(tree, gn, nl, col, T));
    const float p = sig ? sigmoid(z) : fminf(fmaxf(z, 0.f), 1.f);
    const int row = c * kG32Rows + lane;
    const G32RowOut o = g32_row_epilogue<kR, true>(epi, w, M, meta, p, row, n, a.threshold, a.rules, a.proba, a.route);
    emit_flagged(a, o.fr, row);
    // the walk's column reads are done before the next chunk's transpose writes the tile
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
  g32_wave_commit(epi, w, a.counters, lane);
  epi_flush(epi, a.counters);
  signal_done(a, gridDim.x);
}

template <bool kR, bool kG20>
static void launch_fb(const ccfd_score_args& a, hipStream_t s, int grid, int lds_nodes) {
  const size_t lds = kFbFixedLds + (((size_t)lds_nodes * 8 + 15) & ~(size_t)15);
  static const bool opted_in = [] {      // dynamic LDS past 64 KB; the launch itself reports a refusal
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&score_forest_bins_kernel<kR, kG20>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kFbFixedLds + kNodeLdsBytes);
    (void)hipGetLastError();
    return true;
  }();
  (void)opted_in;
  hipLaunchKernelGGL((score_forest_bins_kernel<kR, kG20>), dim3(grid), dim3(256), lds, s, a, lds_nodes);
}

// Grid: one wave per 64-row chunk, capped at 256 x (workgroups per CU) workgroups, grid-stride
// beyond; as many workgroups per CU as the LDS footprint allows (<= 4: 16 waves / CU).
int launch_forest_bins(const ccfd_score_args& a, hipStream_t s) {
  if (a.n <= 0) return 0;
  FrHeader h;
  if (forest_header(a.blob, h) != 0) { set_error("forest launch: cannot read the blob header"); return -2; }
  if (std::memcmp(h.magic, "FRB1", 4) != 0) {
    set_error(std::memcmp(h.magic, "FRS1", 4) == 0
                  ? "forest launch: an FRS1 blob scores f32 rows, these are G32 / G20 rows (pack with bins=)"
                  : "forest launch: not an FRB1 blob");
    return -2;
  }
  if (!forest_shape_ok(h, a)) return -2;
  if (h.stamp < 1 || h.stamp > 255) { set_error("forest launch: FRB1 bin-table stamp outside 1..255"); return -2; }
  const int lds_nodes = (size_t)h.n_nodes * 8 <= (size_t)kNodeLdsBytes ? h.n_nodes : 0;
  const int per_cu = min(4, max(1, (160 * 1024) / (kFbFixedLds + lds_nodes * 8)));
  const int nchunks = (a.n + kG32Rows - 1) / kG32Rows;
  const int grid = min(256 * per_cu, (nchunks + kG32Waves - 1) / kG32Waves);
  const bool r = a.rules != nullptr;
  const bool g20 = (a.flags & CCFD_ARG_WIRE_G20) != 0;
  if (g20 && r) launch_fb<true, true>(a, s, grid, lds_nodes);
  else if (g20) launch_fb<false, true>(a, s, grid, lds_nodes);
  else if (r) launch_fb<true, false>(a, s, grid, lds_nodes);
  else launch_fb<false, false>(a, s, grid, lds_nodes);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace ccfd

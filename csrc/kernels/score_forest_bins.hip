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
//     walked from global memory (L2), and a lane walks several trees at once: the blob view, the
//     staging and the walk are score_forest.hip's (forest_core.h), over this file's FrRowBins;
//   * the scored row goes through the binned kernels' epilogue (g32_row_epilogue: stale stamp
//     -> NaN + CCFD_CNT_WIRE_STALE, amount bucket from the row, proba-only rules) with the
//     blob's link applied here.
//
// All LDS is one dynamic region -- [wave tiles][epilogue][node table] -- so the node table's
// 8- and 16-byte accesses are aligned whatever the compiler does with static LDS.
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

// The lane's row as the walk reads it (forest_core.h fr_walk): `(w & 0x1c) << 4` is dword
// (feat >> 2) * 64 of the lane's column, at most 7 * 64 + 63 of the tile's 512 -- a leaf's
// feature field is 0, so its (ignored) read is in bounds too -- and byte `feat & 3` of it is
// compared with the node's bin index.
struct FrRowBins {
  const unsigned* col;
  __device__ __forceinline__ unsigned fetch(unsigned w) const { return col[(w & 0x1cu) << 4]; }
  __device__ __forceinline__ bool right(unsigned x, const FrNode& nd) const {
    const unsigned bin = (x >> ((nd.w & 3u) * 8u)) & 0xffu;
    return bin > __float_as_uint(nd.v);
  }
};

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

  const FrView m = fr_view(a.blob);
  const G32Model M{nullptr, nullptr, nullptr, m.base, m.stamp};
  const bool resident = m.n_nodes <= lds_nodes;
  if (resident) fr_stage_nodes<256>(m.gn, nl, m.n_nodes, tid);
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

    const FrRowBins bins{col};
    const float z = M.base + (resident ? fr_sum<kFbIlpLds, true, 1>(m, nl, bins, 0)
                                       : fr_sum<kFbIlpGlobal, false, 1>(m, nl, bins, 0));
    const float p = m.sig ? sigmoid(z) : fminf(fmaxf(z, 0.f), 1.f);
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

// Grid: one wave per 64-row chunk, capped at 256 x (workgroups per CU) workgroups, grid-stride
// beyond; as many workgroups per CU as the LDS footprint allows.
int launch_forest_bins(const ccfd_score_args& a, hipStream_t s) {
  if (a.n <= 0) return 0;
  FrLaunch p;
  if (const int rc = forest_prepare(a, "FRB1", "FRS1",
                                    "forest launch: an FRS1 blob scores f32 rows, these are G32 / G20 rows (pack with bins=)",
                                    kFbFixedLds, p))
    return rc;
  if (p.h.stamp < 1 || p.h.stamp > 255) { set_error("forest launch: FRB1 bin-table stamp outside 1..255"); return -2; }
  const int nchunks = (a.n + kG32Rows - 1) / kG32Rows;
  const int grid = min(256 * p.per_cu, (nchunks + kG32Waves - 1) / kG32Waves);
  const size_t lds = kFbFixedLds + (((size_t)p.lds_nodes * 8 + 15) & ~(size_t)15);
  dispatch_bool(a.rules != nullptr, [&](auto r) {
    dispatch_bool((a.flags & CCFD_ARG_WIRE_G20) != 0, [&](auto g20) {
      constexpr auto kernel = &score_forest_bins_kernel<decltype(r)::value, decltype(g20)::value>;
      static const bool opted_in = (fr_lds_opt_in(kernel, kFbFixedLds + kNodeLdsBytes), true);
      (void)opted_in;
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, s, a, p.lds_nodes);
    });
  });
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace ccfd

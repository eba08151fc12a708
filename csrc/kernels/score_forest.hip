// General (non-oblivious) tree ensembles: random forests, sklearn / XGBoost boosted trees
// (models/forest.py, blob 'FRS1').
//
// A general tree has a different split at every node, so a lane's next node depends on its
// own row: the walk is a per-lane gather chain, not the wave-uniform compare-and-shift of
// the oblivious kernels.  Layout per 256-thread workgroup (the v1 oblivious structure):
//   * 64 rows staged FEATURE-MAJOR in LDS (xs[30][64]): lane r reads xs[f][r]; with 64
//     four-byte banks that is bank r for ANY per-lane f, so the divergent feature ids of a
//     general tree cost no bank conflict (rows in VGPRs would need a per-lane register index);
//   * the node table ({u32 w, f32 v} per node, 8 B) staged once per workgroup in dynamic LDS
//     when it fits kNodeLdsBytes, otherwise walked from global memory (it stays L2-resident:
//     every workgroup reads the same few hundred KB);
//   * the 4 waves split the trees (wave w takes trees w, w+4, ...); each lane walks its row
//     through several trees at once, so that many independent gather chains hide each other's
//     latency; partial sums are reduced through LDS, then base + link + threshold / rules +
//     counters + flag list as in the oblivious epilogue.
// The chunk frame (staging, row epilogue) is score_gbdt.hip v1's: gb_rows.h.  The blob view,
// the node staging and the walk are shared with score_forest_bins.hip: forest_core.h, over
// this file's FrRowF32; so is the launch preparation, defined below.
//
// One step of the walk is  next = child + (!leaf && x[feat] > v)  with a leaf's child field
// its own index, so a lane that reached its leaf early stays there while the wave finishes
// the tree's `depth` steps (depth is per tree, a wave-uniform load).
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>

#include "forest_core.h"
#include "gb_rows.h"
#include "rules.h"

namespace ccfd {

void set_error(const std::string& e);

constexpr int kFrStaticLds = 9 * 1024;        // upper bound of this kernel's static LDS (forest_core.h)
// Independent tree walks per lane, measured on 16 M HBM-resident rows (profiles/forest/).
// LDS table (100 complete depth-6 trees): one workgroup per CU is one wave per SIMD and the
// chains are what hides the LDS latency -- 4: 1.85, 8: 2.17, 16: 2.29 G rows/s.  Global table
// (256 random depth-12 trees, 636 KB): up to 16 waves per CU already overlap their L2
// gathers and wider groups lose -- 1: 0.57, 2: 0.39, 4: 0.40 G rows/s.
#ifndef CCFD_FOREST_ILP_LDS
#define CCFD_FOREST_ILP_LDS 8
#endif
#ifndef CCFD_FOREST_ILP_GLOBAL
#define CCFD_FOREST_ILP_GLOBAL 1
#endif
constexpr int kIlpLds = CCFD_FOREST_ILP_LDS;
constexpr int kIlpGlobal = CCFD_FOREST_ILP_GLOBAL;

// The lane's row as the walk reads it (forest_core.h fr_walk): feature `w & 31` of column
// `lane` of the feature-major tile, and `x > v`.
struct FrRowF32 {
  const float (*xs)[kGbRows];
  int lane;
  __device__ __forceinline__ float fetch(unsigned w) const { return xs[w & 31u][lane]; }
  __device__ __forceinline__ bool right(float x, const FrNode& nd) const { return x > nd.v; }
};

// `lds_nodes`: nodes the launch allocated dynamic LDS for (0 = none).  T, n_nodes and the
// link come from the blob's own header, so what bounds every read is the blob itself.
template <bool kContig, bool kR>
__global__ __launch_bounds__(256) void score_forest_kernel(ccfd_score_args a, int cpw, int lds_nodes) {
  __shared__ __attribute__((aligned(16))) float xs[kF][kGbRows];
  extern __shared__ __attribute__((aligned(16))) uint2 nl[];   // lds_nodes nodes (rounded up to 16 B)
  __shared__ float part[kGbWaves][kGbRows];
  __shared__ EpilogueLds epi;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nchunks = (a.n + kGbRows - 1) / kGbRows;
  const int c_begin = blockIdx.x * cpw;
  const int c_end = min(nchunks, c_begin + cpw);
  epi_init(epi);
  stamp_start(a, blockIdx.x);

  const FrView m = fr_view(a.blob);
  const bool resident = m.n_nodes <= lds_nodes;

  GbRegs cur, nxt;
  if constexpr (kContig)
    if (c_begin < c_end) gb_issue(a.x, c_begin * kGbRows, min(kGbRows, a.n - c_begin * kGbRows), tid, cur);

  if (resident) fr_stage_nodes<256>(m.gn, nl, m.n_nodes, tid);    // visible after the first loop barrier

  for (int c = c_begin; c < c_end; ++c) {
    const int row0 = c * kGbRows;
    const int nrows = min(kGbRows, a.n - row0);
    __syncthreads();   // previous chunk's xs / part readers are done
    gb_stage<kContig>(a, xs, tid, row0, nrows, c + 1 < c_end, cur, nxt);
    __syncthreads();     // rows (and nodes) staged

    // this wave's trees: wave, wave + 4, ...
    const FrRowF32 row{xs, lane};
    part[wave][lane] = resident ? fr_sum<kIlpLds, true, kGbWaves>(m, nl, row, wave)
                                : fr_sum<kIlpGlobal, false, kGbWaves>(m, nl, row, wave);
    __syncthreads();

    if (wave == 0) {
      const float z = m.base + part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
      const float p = m.sig ? sigmoid(z) : fminf(fmaxf(z, 0.f), 1.f);
      gb_row_epilogue<kR>(a, epi, xs, p, lane, row0, nrows);
    }
    if constexpr (kContig) cur = nxt;
  }
  epi_flush(epi, a.counters);
  signal_done(a, gridDim.x);
}

// The cache of blob headers of both general-tree launches (forest_core.h).
static std::mutex g_fr_mu;
static std::unordered_map<const void*, FrHeader> g_fr_headers;

int forest_header(const void* blob, FrHeader& h) {
  std::lock_guard<std::mutex> g(g_fr_mu);
  auto it = g_fr_headers.find(blob);
  if (it != g_fr_headers.end()) { h = it->second; return 0; }
  if (hipMemcpy(&h, blob, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (g_fr_headers.size() >= 256) g_fr_headers.clear();
  g_fr_headers.emplace(blob, h);
  return 0;
}

bool forest_shape_ok(const FrHeader& h, const ccfd_score_args& a) {
  if (h.T <= 0 || a.gbdt_trees <= 0) { set_error("forest launch: no trees"); return false; }
  if (h.depth < 0 || h.depth > kFrMaxDepth || a.gbdt_depth < 0 || a.gbdt_depth > kFrMaxDepth) {
    set_error("forest launch: tree depth outside 0..64");
    return false;
  }
  if (h.n_nodes < h.T || h.n_nodes >= kFrMaxNodes) { set_error("forest launch: node count outside [T, 2^24)"); return false; }
  return true;
}

int forest_prepare(const ccfd_score_args& a, const char* magic, const char* other, const char* other_hint,
                   int fixed_lds, FrLaunch& p) {
  if (forest_header(a.blob, p.h) != 0) { set_error("forest launch: cannot read the blob header"); return -2; }
  if (std::memcmp(p.h.magic, magic, 4) != 0) {
    set_error(std::memcmp(p.h.magic, other, 4) == 0 ? std::string(other_hint)
                                                    : std::string("forest launch: not an ") + magic + " blob");
    return -2;
  }
  if (!forest_shape_ok(p.h, a)) return -2;
  p.lds_nodes = (size_t)p.h.n_nodes * 8 <= (size_t)kNodeLdsBytes ? p.h.n_nodes : 0;
  p.per_cu = min(4, max(1, (160 * 1024) / (fixed_lds + p.lds_nodes * 8)));
  return 0;
}

int launch_forest(const ccfd_score_args& a, hipStream_t s) {
  if (a.n <= 0) return 0;
  FrLaunch p;
  if (const int rc = forest_prepare(a, "FRS1", "FRB1",
                                    "forest launch: an FRB1 blob scores G32 / G20 rows, these are f32 rows (pack without bins=)",
                                    kFrStaticLds, p))
    return rc;
  const bool contig = a.ld == kF && (reinterpret_cast<uintptr_t>(a.x) & 15) == 0;
  // ~one wave of workgroups: as many per CU as the LDS footprint allows
  const int nchunks = (a.n + kGbRows - 1) / kGbRows;
  const int cpw = max(1, (nchunks + 256 * p.per_cu - 1) / (256 * p.per_cu));
  const int grid = (nchunks + cpw - 1) / cpw;
  const size_t lds = ((size_t)p.lds_nodes * 8 + 15) & ~(size_t)15;
  dispatch_bool(contig, [&](auto c) {
    dispatch_bool(a.rules != nullptr, [&](auto r) {
      constexpr auto kernel = &score_forest_kernel<decltype(c)::value, decltype(r)::value>;
      static const bool opted_in = (fr_lds_opt_in(kernel, kNodeLdsBytes), true);
      (void)opted_in;
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, s, a, cpw, p.lds_nodes);
    });
  });
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace ccfd

extern "C" void ccfd_forest_blob_changed(const void* blob) {
  std::lock_guard<std::mutex> g(ccfd::g_fr_mu);
  ccfd::g_fr_headers.erase(blob);
}

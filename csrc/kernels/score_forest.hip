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

// Walk U trees (t0, t0 + 4, ...) of this wave for the lane's row; returns the leaf sum.
// The step is branch-free on purpose: a leaf's feature field is 0, so its (ignored) feature
// read is in bounds, and the U chains' loads stay interleaved -- a short-circuit `&&` here
// compiles to one exec-masked branch per chain, each waiting for its own LDS read.
template <int U, bool kLds>
__device__ __forceinline__ float fr_walk(const int* __restrict__ tree, const uint2* __restrict__ gn, const uint2* ln,
                                         const float (*xs)[kGbRows], int lane, int t0) {
  FrNode nd[U];
  int depth = 0;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int t = t0 + kGbWaves * u;
    const unsigned root = (unsigned)__builtin_amdgcn_readfirstlane(tree[2 * t]);
    depth = max(depth, __builtin_amdgcn_readfirstlane(tree[2 * t + 1]));
    nd[u] = fr_node<kLds>(gn, ln, root);
  }
  for (int s = 0; s < depth; ++s) {
    float x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) x[u] = xs[nd[u].w & 31u][lane];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned inner = ((nd[u].w >> 5) & 1u) ^ 1u;
      const unsigned gt = x[u] > nd[u].v ? 1u : 0u;
      nd[u] = fr_node<kLds>(gn, ln, (nd[u].w >> 8) + (gt & inner));
    }
  }
  float acc = 0.f;
#pragma unroll
  for (int u = 0; u < U; ++u) acc += nd[u].v;
  return acc;
}

// This wave's trees, kU at a time, then the tail in halving group sizes (a single-tree walk
// costs the latency of a full group).
template <int U, bool kLds>
__device__ __forceinline__ void fr_tail(const int* __restrict__ tree, const uint2* __restrict__ gn, const uint2* ln,
                                        const float (*xs)[kGbRows], int lane, int T, int& t, float& acc) {
  if (t + kGbWaves * (U - 1) < T) { acc += fr_walk<U, kLds>(tree, gn, ln, xs, lane, t); t += kGbWaves * U; }
  if constexpr (U > 1) fr_tail<U / 2, kLds>(tree, gn, ln, xs, lane, T, t, acc);
}

template <bool kLds>
__device__ __forceinline__ float fr_wave_sum(const int* __restrict__ tree, const uint2* __restrict__ gn,
                                             const uint2* ln, const float (*xs)[kGbRows], int lane, int wave, int T) {
  constexpr int kU = kLds ? kIlpLds : kIlpGlobal;
  static_assert((kU & (kU - 1)) == 0, "group sizes halve down to 1");
  float acc = 0.f;
  int t = wave;
  for (; t + kGbWaves * (kU - 1) < T; t += kGbWaves * kU) acc += fr_walk<kU, kLds>(tree, gn, ln, xs, lane, t);
  if constexpr (kU > 1) fr_tail<kU / 2, kLds>(tree, gn, ln, xs, lane, T, t, acc);
  return acc;
}

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

  const char* blob = reinterpret_cast<const char*>(a.blob);
  const int* __restrict__ hdr = reinterpret_cast<const int*>(blob);
  const bool sig = (hdr[1] & 1) != 0;
  const int T = hdr[2];
  const float base = *reinterpret_cast<const float*>(blob + 16);
  const int n_nodes = hdr[5];
  const int* __restrict__ tree = reinterpret_cast<const int*>(blob + kHeader);
  const uint2* __restrict__ gn = reinterpret_cast<const uint2*>(blob + kHeader + ((8 * (size_t)T + 15) & ~(size_t)15));
  const bool resident = n_nodes <= lds_nodes;

  GbRegs cur, nxt;
  if constexpr (kContig)
    if (c_begin < c_end) gb_issue(a.x, c_begin * kGbRows, min(kGbRows, a.n - c_begin * kGbRows), tid, cur);

  if (resident) {     // 16-byte copies: the node section is padded to 16 B; visible after the first loop barrier
    const uint4* s4 = reinterpret_cast<const uint4*>(gn);
    uint4* d4 = reinterpret_cast<uint4*>(nl);
    for (int i = tid; i < (n_nodes + 1) / 2; i += 256) d4[i] = ld_g16(s4 + i);
  }

  for (int c = c_begin; c < c_end; ++c) {
    const int row0 = c * kGbRows;
    const int nrows = min(kGbRows, a.n - row0);
    __syncthreads();   // previous chunk's xs / part readers are done
    if constexpr (kContig) {
      if (c + 1 < c_end) gb_issue(a.x, row0 + kGbRows, min(kGbRows, a.n - row0 - kGbRows), tid, nxt);
      gb_store(xs, tid, cur);
    } else {
      for (int e = tid; e < kGbRows * kF; e += 256) {
        const int r = e / kF, f = e % kF;
        xs[f][r] = (r < nrows) ? a.x[(size_t)(row0 + r) * a.ld + f] : 0.f;
      }
    }
    __syncthreads();     // rows (and nodes) staged

    part[wave][lane] = resident ? fr_wave_sum<true>(tree, gn, nl, xs, lane, wave, T)
                                : fr_wave_sum<false>(tree, gn, nl, xs, lane, wave, T);
    __syncthreads();

    if (wave == 0) {
      const float z = base + part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
      const float p = sig ? sigmoid(z) : fminf(fmaxf(z, 0.f), 1.f);
      const bool valid = lane < nrows;
      bool fr;
      if constexpr (kR) fr = valid && rule_route(a.rules, p, [&](int j) { return xs[j][lane]; });
      else fr = valid && (p >= a.threshold);
      const int row = row0 + lane;
      if (valid) {
        if (a.proba) st_g(a.proba + row, p);
        if (a.route) st_g(a.route + row, (uint8_t)(fr ? 1 : 0));
        atomicAdd(&epi.hist[(fr ? kNB : 0) + amount_bucket(xs[kAmountCol][lane])], 1u);
      }
      unsigned long long ps = valid ? (unsigned long long)(p * 1e6f + 0.5f) : 0ull;
      ps = wave_sum_u64(ps);
      const unsigned nf = __popcll(__ballot(fr));
      if (lane == 0) { epi.fraud += nf; epi.rows += nrows; epi.psum_e6 += ps; }
      emit_flagged(a, fr, row);
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

template <bool kContig, bool kR>
static void launch_fr(const ccfd_score_args& a, hipStream_t s, int grid, int cpw, int lds_nodes) {
  const size_t lds = ((size_t)lds_nodes * 8 + 15) & ~(size_t)15;
  static const bool opted_in = [] {      // dynamic LDS past 64 KB; the launch itself reports a refusal
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&score_forest_kernel<kContig, kR>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kNodeLdsBytes);
    (void)hipGetLastError();
    return true;
  }();
  (void)opted_in;
  hipLaunchKernelGGL((score_forest_kernel<kContig, kR>), dim3(grid), dim3(256), lds, s, a, cpw, lds_nodes);
}

int launch_forest(const ccfd_score_args& a, hipStream_t s) {
  if (a.n <= 0) return 0;
  FrHeader h;
  if (forest_header(a.blob, h) != 0) { set_error("forest launch: cannot read the blob header"); return -2; }
  if (std::memcmp(h.magic, "FRS1", 4) != 0) {
    set_error(std::memcmp(h.magic, "FRB1", 4) == 0
                  ? "forest launch: an FRB1 blob scores G32 / G20 rows, these are f32 rows (pack without bins=)"
                  : "forest launch: not an FRS1 blob");
    return -2;
  }
  if (!forest_shape_ok(h, a)) return -2;
  const bool contig = a.ld == kF && (reinterpret_cast<uintptr_t>(a.x) & 15) == 0;
  const int lds_nodes = (size_t)h.n_nodes * 8 <= (size_t)kNodeLdsBytes ? h.n_nodes : 0;
  // ~one wave of workgroups: as many per CU as the LDS footprint allows (<= 4: 16 waves / CU)
  const int per_cu = min(4, max(1, (160 * 1024) / (kFrStaticLds + lds_nodes * 8)));
  const int nchunks = (a.n + kGbRows - 1) / kGbRows;
  const int cpw = max(1, (nchunks + 256 * per_cu - 1) / (256 * per_cu));
  const int grid = (nchunks + cpw - 1) / cpw;
  const bool r = a.rules != nullptr;
  if (contig && r) launch_fr<true, true>(a, s, grid, cpw, lds_nodes);
  else if (contig) launch_fr<true, false>(a, s, grid, cpw, lds_nodes);
  else if (r) launch_fr<false, true>(a, s, grid, cpw, lds_nodes);
  else launch_fr<false, false>(a, s, grid, cpw, lds_nodes);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace ccfd

extern "C" void ccfd_forest_blob_changed(const void* blob) {
  std::lock_guard<std::mutex> g(ccfd::g_fr_mu);
  ccfd::g_fr_headers.erase(blob);
}

// Exact per-feature Shapley values of an oblivious GBDT on G32 rows (path-dependent TreeSHAP,
// margin space; the definition is in docs/EXPLAIN.md and models/explain.py, whose
// shapley_oblivious is the oracle and whose ExplainTable.pack writes the 'GBX1' blob read here).
//
// One row per lane, trees wave-uniform.  A workgroup is 4 waves that share the same 64 rows
// and split the trees between them (tree tt of a staged block goes to wave tt % 4), so a small
// batch still spreads over many SIMDs; every wave keeps its own 30 accumulators a lane in LDS
// and the four are added in a fixed order at the end.  Per tree and per subset S of its m
// distinct features the value function is the restricted leaf sum
//   v(S) = sum over leaves l that agree with the row on the levels of S of
//          leaves[l] * prod_{d not in S} frac_d(l)
// (3^D leaf terms a tree when all levels test different features), and
//   phi_j = sum_S c_j(S) v(S),  c_j(S) = w[m][|S|-1] if j in S else -w[m][|S|].
// Everything that does not depend on the row -- the subset, its level mask, the enumeration of
// the free levels' leaves, the per-level table offsets, the Shapley coefficients -- is
// wave-uniform and lives in SGPRs (a tree's 48 descriptor words arrive as one vector load and
// are read out by lane); the row enters through its leaf index only.  The leaf and fraction
// tables of a block of trees are staged in LDS and read by per-lane gathers.  A leaf term is
// branch-free: a level that S fixes reads the table's spare entry, which is marked empty, and
// "follow the row" makes its factor exactly 1; so the D gathers of a term are independent, and
// four terms are in flight at a time (the first version walked the free levels in a loop and
// waited for LDS at every level: 18.6 ms for 64 rows of the 100 x 6 model on one wave).
// The row's bytes are staged as rowb[word][lane] and the accumulators as phi[wave][feature][lane],
// both indexed by a wave-uniform word / feature: conflict-free, no atomics, nothing in scratch.
// v(S) and the per-tree Shapley sums accumulate in f64 (2^D + m 2^m adds a tree against
// ~D 3^D f32 multiplies); products and the per-feature totals are f32.  The order of every sum
// is fixed and does not depend on n: results are bit-identical from run to run.
#include <algorithm>
#include <string>

#include "common.h"

namespace ccfd {

void set_error(const std::string& e);

constexpr int kExplainWaves = 4;
constexpr int kExplainThreads = 64 * kExplainWaves;
constexpr int kExplainTabFloats = 4096;      // 16 KiB of leaf + fraction tables a tree block
constexpr int kExplainTerms = 4;             // leaf terms in flight
constexpr int kGbxMeta = CCFD_GBX_META_WORDS;
constexpr int kGbxWeights = CCFD_GBX_WEIGHT_BYTES / 8;

struct ExplainLds {
  float phi[kExplainWaves * kF * 64];        // [wave][feature][lane]
  unsigned rowb[8 * 64];                     // [word of the G32 row][lane]
  float tab[kExplainTabFloats];              // [c][2^D] leaves, then [c][2^(D+1)] fractions
  double w[kGbxWeights];                     // Shapley weights w[m][s]
};                                           // 49.7 KiB: three workgroups a CU

template <int D>
__device__ __forceinline__ float leaf_term(const float* lv, const float* fr, unsigned l, unsigned lx,
                                           const unsigned (&off)[D], const unsigned (&msk)[D]) {
  float f[D];
  float p = lv[l];
#pragma unroll
  for (int d = 0; d < D; ++d) f[d] = fr[off[d] + (l & msk[d])];
  const unsigned off_row = l ^ lx;                     // bit d set: l leaves the row's path at level d
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const float follow = (off_row >> d) & 1u ? 0.f : 1.f;
    p *= f[d] < 0.f ? follow : f[d];                   // no background row at the parent: follow the row
  }
  return p;
}

template <int D>
__global__ __launch_bounds__(kExplainThreads) void gbdt_explain_kernel(ccfd_gbdt_explain_args a, int chunk) {
  __shared__ __attribute__((aligned(16))) ExplainLds s;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t row0 = (int64_t)blockIdx.x * 64;
  const int T = a.trees;
  constexpr int nleaf = 1 << D, nfrac = 2 << D;
  constexpr unsigned full = (unsigned)nleaf - 1u;
  constexpr unsigned spare = (unsigned)nfrac - 2u;     // marked empty by the packer

  const uint8_t* blob = static_cast<const uint8_t*>(a.blob);
  const int stamp = __builtin_amdgcn_readfirstlane(ld_g(reinterpret_cast<const int32_t*>(blob + 20)));
  const double* wtab = reinterpret_cast<const double*>(blob + kHeader);
  const int32_t* meta = reinterpret_cast<const int32_t*>(blob + kHeader + CCFD_GBX_WEIGHT_BYTES);
  const float* g_leaves = reinterpret_cast<const float*>(meta + (size_t)T * kGbxMeta);
  const float* g_frac = g_leaves + ((size_t)T << D);

  if (tid < 64) {
    uint4 lo = make_uint4(0u, 0u, 0u, 0u), hi = lo;
    if (row0 + lane < a.n) {
      lo = ld_g16(a.rows + (row0 + lane) * CCFD_G32_ROW_BYTES);
      hi = ld_g16(a.rows + (row0 + lane) * CCFD_G32_ROW_BYTES + 16);
    }
    s.rowb[0 * 64 + lane] = lo.x; s.rowb[1 * 64 + lane] = lo.y;
    s.rowb[2 * 64 + lane] = lo.z; s.rowb[3 * 64 + lane] = lo.w;
    s.rowb[4 * 64 + lane] = hi.x; s.rowb[5 * 64 + lane] = hi.y;
    s.rowb[6 * 64 + lane] = hi.z; s.rowb[7 * 64 + lane] = hi.w;
  } else if (tid < 64 + kGbxWeights) {
    s.w[tid - 64] = ld_g(wtab + (tid - 64));
  }
  for (int i = tid; i < kExplainWaves * kF * 64; i += kExplainThreads) s.phi[i] = 0.f;
  float* phi = s.phi + wave * (kF * 64);

  for (int t0 = 0; t0 < T; t0 += chunk) {
    const int c = min(chunk, T - t0);
    __syncthreads();                                   // the previous block's gathers are done
    for (int i = tid; i < c * nleaf; i += kExplainThreads) s.tab[i] = ld_g(g_leaves + ((size_t)t0 << D) + i);
    for (int i = tid; i < c * nfrac; i += kExplainThreads)
      s.tab[c * nleaf + i] = ld_g(g_frac + ((size_t)t0 << (D + 1)) + i);
    __syncthreads();

    for (int tt = wave; tt < c; tt += kExplainWaves) {
      // the tree's descriptor: one load, lane i holds word i
      const int mv = ld_g(meta + (size_t)(t0 + tt) * kGbxMeta + (lane < kGbxMeta ? lane : 0));
      const float* lv = s.tab + tt * nleaf;
      const float* fr = s.tab + c * nleaf + tt * nfrac;
      const int m = max(0, min(__builtin_amdgcn_readlane(mv, 40), 8));   // clamps: a damaged blob stays inside LDS
      int slot_mask[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) slot_mask[j] = __builtin_amdgcn_readlane(mv, 32 + j);

      unsigned lx = 0;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const int f = __builtin_amdgcn_readlane(mv, d) & 31, k = __builtin_amdgcn_readlane(mv, 8 + d);
        const unsigned b = (s.rowb[(f >> 2) * 64 + lane] >> ((f & 3) * 8)) & 0xffu;
        lx |= (b > (unsigned)k ? 1u : 0u) << d;
      }

      double acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.0;

      for (int sm = 0; sm < (1 << m); ++sm) {          // subsets of the tree's features
        unsigned lmask = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) lmask |= (sm >> j) & 1 ? (unsigned)slot_mask[j] : 0u;
        const unsigned free_lv = ~lmask & full;
        const unsigned fixed = lx & lmask;
        const int sz = __builtin_popcount((unsigned)sm);
        const double c_in = sz > 0 ? s.w[m * 8 + (sz - 1)] : 0.0;
        const double c_out = sz < m ? -s.w[m * 8 + sz] : 0.0;
        unsigned off[D], msk[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
          const bool is_free = (free_lv >> d) & 1u;
          off[d] = is_free ? (2u << d) - 2u : spare;
          msk[d] = is_free ? (2u << d) - 1u : 0u;
        }
        double v = 0.0;
        unsigned sub = free_lv;                        // leaves over the free levels, descending
        bool more = true;
        while (more) {
          unsigned l[kExplainTerms];
          bool live[kExplainTerms];
#pragma unroll
          for (int q = 0; q < kExplainTerms; ++q) {
            l[q] = fixed | sub;
            live[q] = more;
            if (sub == 0u) more = false;
            sub = (sub - 1u) & free_lv;
          }
          float p[kExplainTerms];
#pragma unroll
          for (int q = 0; q < kExplainTerms; ++q) p[q] = leaf_term<D>(lv, fr, l[q], lx, off, msk);
#pragma unroll
          for (int q = 0; q < kExplainTerms; ++q) v += (double)(live[q] ? p[q] : 0.f);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (j < m) acc[j] = fma(v, (sm >> j) & 1 ? c_in : c_out, acc[j]);
      }

#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < m) {
          const int f = min(__builtin_amdgcn_readlane(mv, 24 + j) & 31, kF - 1);
          phi[f * 64 + lane] += (float)acc[j];
        }
    }
  }

  __syncthreads();
  // the workgroup's rows are 64 * 30 contiguous floats of the output: store them coalesced
  const int nrow = (int)min((int64_t)64, a.n - row0);
  float* out = a.phi + row0 * kF;
  for (int e = tid; e < nrow * kF; e += kExplainThreads) {
    const int r = e / kF, f = e - r * kF;
    float v = s.phi[f * 64 + r];
#pragma unroll
    for (int w = 1; w < kExplainWaves; ++w) v += s.phi[w * (kF * 64) + f * 64 + r];
    if (((s.rowb[7 * 64 + r] >> 24) & 0xffu) != (unsigned)stamp)
      v = __uint_as_float(0x7fc00000u);                // a stale row is not an explanation
    st_g(out + e, v);
  }
}

template <int D>
static void launch_explain(const ccfd_gbdt_explain_args& a, int chunk, hipStream_t s) {
  hipLaunchKernelGGL(gbdt_explain_kernel<D>, dim3((unsigned)((a.n + 63) / 64)), dim3(kExplainThreads), 0, s, a, chunk);
}

}  // namespace ccfd

extern "C" int ccfd_gbdt_explain_launch(const ccfd_gbdt_explain_args* a, void* stream) {
  using namespace ccfd;
  if (a == nullptr) { set_error("gbdt explain: null argument"); return -1; }
  if (a->trees < 1) { set_error("gbdt explain: trees < 1"); return -2; }
  if (a->depth < 1 || a->depth > CCFD_GBDT_MAX_SPLITS) { set_error("gbdt explain: depth outside 1..8"); return -2; }
  if (a->n < 0) { set_error("gbdt explain: n < 0"); return -2; }
  if (a->n > (int64_t)0x7fffffff * 64) { set_error("gbdt explain: n too large for one launch"); return -2; }
  const int64_t need = (int64_t)kHeader + CCFD_GBX_WEIGHT_BYTES +
                       (int64_t)a->trees * (4 * kGbxMeta + ((int64_t)12 << a->depth));
  if (a->blob_bytes < need) { set_error("gbdt explain: blob smaller than a GBX1 blob of this shape"); return -2; }
  if (a->n == 0) return 0;
  if (a->rows == nullptr || a->blob == nullptr || a->phi == nullptr) {
    set_error("gbdt explain: null argument");
    return -1;
  }
  if (reinterpret_cast<uintptr_t>(a->rows) & 15) { set_error("gbdt explain: G32 rows must be 16-byte aligned"); return -3; }
  if (reinterpret_cast<uintptr_t>(a->blob) & 15) { set_error("gbdt explain: the blob must be 16-byte aligned"); return -3; }
  // trees staged at a time: what fits the table budget, a multiple of the waves that share them
  const int per_tree = 3 << a->depth;                  // 2^D leaves + 2^(D+1) fractions
  int chunk = std::max(1, kExplainTabFloats / per_tree);
  if (chunk >= kExplainWaves) chunk -= chunk % kExplainWaves;
  chunk = std::min(chunk, (int)a->trees);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  dispatch_depth(a->depth, [&](auto d) { launch_explain<decltype(d)::value>(*a, chunk, s); });
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
    set_error(std::string("gbdt explain: launch failed: ") + hipGetErrorString(e));
    return -5;
  }
  return 0;
}

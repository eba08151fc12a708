// Exact per-feature Shapley values of a general tree ensemble on G32 rows (path-dependent
// TreeSHAP of the raw score; the definition is in docs/EXPLAIN.md and models/explain_forest.py,
// whose shapley_forest is the oracle and whose ForestExplainTable.pack writes the 'FRX1' blob
// read here: one record per root-to-leaf path).
//
// explain_gbdt's shape: one row per lane, everything else wave-uniform.  A workgroup is 4 waves
// that share the same 64 rows; the blob cuts its paths into slices and every slice into one run
// of records per wave.  A record does not depend on the row: the wave reads it with one vector
// load (lane i holds word i) and takes the words out by lane into SGPRs, and the next record's
// load is in flight while this one is worked on; the table stays in global memory / L2.  On
// one path the m <= W players (the path's splits merged per feature: a bin interval and the
// product z of the background shares) are, per lane, satisfied (o = 1) or not (o = 0), and
//   phi[f_e] += leaf * gate * (o_e - z_e) * int_0^1 prod_{i != e} (o_i t + z_i (1 - t)) dt
// (the Shapley weight k! (m-k-1)! / m! is the integral of t^k (1-t)^(m-k-1)).  The integrand has
// degree m - 1, so the blob's Gauss-Legendre rule of ceil(m / 2) nodes is exact; the kernel is
// instantiated per width bucket W of the blob and everything is indexed statically.  At a node
// the factors live in VGPRs and the product without e is a running prefix times a stored
// suffix: nothing divides (z may be exactly 0), every factor is in [0, 1] and every term is
// >= 0, so nothing cancels either.  (Expanding the product into coefficients and taking one
// factor out again by synthetic division, as the float64 oracle does, loses the small end
// coefficients in f32: 80 u of local-accuracy error on a 16-player chain against 3.7 u here.)
// Per lane only the satisfied mask varies, and it enters through selects, not branches; a slot
// past m is the null player o = z = 1, and wave-uniform branches skip its work.
// The row's bytes are staged as rowb[word][lane] and the accumulators as phi[wave][feature][lane],
// both indexed by a wave-uniform word / feature: conflict-free, no atomics, nothing in scratch.
//
// Order of the sums: the records of a wave's run in table order; the 4 waves of a slice as
// ((w0 + w1) + w2) + w3; the slices in order, from 0.  A batch of few rows runs the slices on
// grid.y and a second kernel adds their partial sums in that same order, so the bits of a row
// depend on neither n nor its neighbours, and two runs give the same bits.
#include <algorithm>
#include <string>

#include "common.h"

namespace ccfd {

void set_error(const std::string& e);

constexpr int kFrxWaves = CCFD_FRX_WAVES;
constexpr int kFrxThreads = 64 * kFrxWaves;
constexpr int kFrxRule = CCFD_FRX_RULE_BYTES / 8;          // [q - 1][nodes, weights][8]: the q-point rules
constexpr int kFrxMaxGates = 64;

struct ForestExplainLds {
  float phi[kFrxWaves * kF * 64];            // [wave][feature][lane]
  float tot[kF * 64];                        // [feature][lane]: the slices so far
  unsigned rowb[8 * 64];                     // [word of the G32 row][lane]
  float rule[kFrxRule];                      // the quadrature rules
};                                           // 40.0 KiB: three workgroups a CU

__device__ __forceinline__ unsigned frx_lane(unsigned v, int i) { return (unsigned)__builtin_amdgcn_readlane((int)v, i); }

// lo < bin <= hi of the feature in word `pw` (feature | (lo + 1) << 8 | hi << 20), for this lane's row
__device__ __forceinline__ bool frx_inside(const unsigned* rowb, int lane, unsigned pw) {
  const unsigned f = min(pw & 31u, (unsigned)(kF - 1));
  const unsigned b = (rowb[(f >> 2) * 64 + lane] >> ((f & 3u) * 8u)) & 0xffu;
  return b >= ((pw >> 8) & 0x1ffu) && b <= ((pw >> 20) & 0xffu);
}

// One record, whose words [0, 64) are in h0 and [64, 128) in h1 (lane i: word i).
template <int W>
__device__ __forceinline__ void explain_record(unsigned h0, unsigned h1, int m, int ng, const unsigned* rowb,
                                               const float* rule, float* phi, int lane) {
  float lead = __uint_as_float(frx_lane(h0, 0));             // leaf value, 0 for a row the gates stop
  for (int g = 0; g < ng; ++g) {
    const int at = 2 + 2 * m + g;
    const unsigned gw = at < 64 ? frx_lane(h0, at) : frx_lane(h1, at - 64);
    lead = frx_inside(rowb, lane, gw) ? lead : 0.f;
  }
  float z[W], acc[W];
  bool sat[W];
  unsigned pw[W];
#pragma unroll
  for (int i = 0; i < W; ++i) {
    pw[i] = frx_lane(h0, 2 + 2 * i);
    z[i] = __uint_as_float(frx_lane(h0, 3 + 2 * i));
    sat[i] = i < m && frx_inside(rowb, lane, pw[i]);
    acc[i] = 0.f;
  }
  const int nq = max(1, (m + 1) >> 1);                       // nodes that integrate degree m - 1 exactly
  const float* rl = rule + (nq - 1) * 16;
#pragma unroll 1
  for (int j = 0; j < nq; ++j) {                             // one node at a time: W factors and W suffixes live
    const float t = rl[j], om = rl[8 + j], u = 1.f - t;
    float f[W], suf[W];
#pragma unroll
    for (int i = 0; i < W; ++i) {
      const float zu = z[i] * u;
      f[i] = i < m ? (sat[i] ? zu + t : zu) : 1.f;
    }
    suf[W - 1] = 1.f;
#pragma unroll
    for (int i = W - 1; i >= 1; --i) suf[i - 1] = suf[i] * f[i];
    float pre = 1.f;
#pragma unroll
    for (int e = 0; e < W; ++e)
      if (e < m) {
        acc[e] = fmaf(om, pre * suf[e], acc[e]);
        pre *= f[e];
      }
  }
#pragma unroll
  for (int e = 0; e < W; ++e)
    if (e < m) {
      const int fe = (int)min(pw[e] & 31u, (unsigned)(kF - 1));
      phi[fe * 64 + lane] += (lead * ((sat[e] ? 1.f : 0.f) - z[e])) * acc[e];
    }
}

template <int W>
__global__ __launch_bounds__(kFrxThreads) void forest_explain_kernel(ccfd_forest_explain_args a, int slices_per_block) {
  __shared__ __attribute__((aligned(16))) ForestExplainLds s;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t row0 = (int64_t)blockIdx.x * 64;
  const int S = a.slices, R = a.rec_words;

  const uint8_t* blob = static_cast<const uint8_t*>(a.blob);
  const int stamp = __builtin_amdgcn_readfirstlane(ld_g(reinterpret_cast<const int32_t*>(blob + 20)));
  const double* rule = reinterpret_cast<const double*>(blob + kHeader);
  const int32_t* seg = reinterpret_cast<const int32_t*>(blob + kHeader + CCFD_FRX_RULE_BYTES);
  const unsigned* rec = reinterpret_cast<const unsigned*>(seg + (size_t)S * kFrxWaves * 2);

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
  }
  if (tid >= 64 && tid < 64 + kFrxRule) s.rule[tid - 64] = (float)ld_g(rule + (tid - 64));   // 128 values, 192 threads
  for (int i = tid; i < kFrxWaves * kF * 64; i += kFrxThreads) s.phi[i] = 0.f;
  for (int i = tid; i < kF * 64; i += kFrxThreads) s.tot[i] = 0.f;
  float* phi = s.phi + wave * (kF * 64);
  __syncthreads();

  const int s0 = (int)blockIdx.y * slices_per_block, s1 = min(S, s0 + slices_per_block);
  for (int sl = s0; sl < s1; ++sl) {
    const int32_t* sg = seg + ((size_t)sl * kFrxWaves + wave) * 2;
    int off = __builtin_amdgcn_readfirstlane(ld_g(sg));
    int cnt = __builtin_amdgcn_readfirstlane(ld_g(sg + 1));
    if (R < 1 || off < 0 || off >= R) cnt = 0;                 // clamps: a damaged blob stays inside the table
    unsigned h0 = 0u, h1 = 0u;
    if (cnt > 0) {
      h0 = ld_g(rec + min(off + lane, R - 1));
      h1 = ld_g(rec + min(off + 64 + lane, R - 1));
    }
    for (int p = 0; p < cnt; ++p) {
      const unsigned mw = frx_lane(h0, 1);
      const int m = min((int)(mw & 0xffu), W), ng = min((int)((mw >> 8) & 0xffu), kFrxMaxGates);
      const unsigned c0 = h0, c1 = h1;
      off += 2 + 2 * m + ng + (ng & 1);
      if (off >= R) cnt = 0;                                   // the last record, or a damaged length
      if (p + 1 < cnt) {                                       // the next record, while this one is worked on
        h0 = ld_g(rec + min(off + lane, R - 1));
        h1 = ld_g(rec + min(off + 64 + lane, R - 1));
      }
      explain_record<W>(c0, c1, m, ng, s.rowb, s.rule, phi, lane);
    }
    __syncthreads();
    for (int i = tid; i < kF * 64; i += kFrxThreads) {
      float v = s.phi[i];
#pragma unroll
      for (int w = 1; w < kFrxWaves; ++w) v += s.phi[w * (kF * 64) + i];
      s.tot[i] += v;
#pragma unroll
      for (int w = 0; w < kFrxWaves; ++w) s.phi[w * (kF * 64) + i] = 0.f;
    }
    __syncthreads();
  }

  // the workgroup's rows are 64 * 30 contiguous floats of the output: store them coalesced
  const int nrow = (int)min((int64_t)64, a.n - row0);
  float* out = (gridDim.y == 1 ? a.phi : a.workspace + (int64_t)blockIdx.y * a.n * kF) + row0 * kF;
  for (int e = tid; e < nrow * kF; e += kFrxThreads) {
    const int r = e / kF, f = e - r * kF;
    float v = s.tot[f * 64 + r];
    if (((s.rowb[7 * 64 + r] >> 24) & 0xffu) != (unsigned)stamp)
      v = __uint_as_float(0x7fc00000u);                // a stale row is not an explanation
    st_g(out + e, v);
  }
}

// phi = the slices' partial sums, added in slice order from 0 (NaN of a stale row carries through)
__global__ __launch_bounds__(256) void forest_explain_sum_kernel(const float* part, float* phi, int64_t total, int slices) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  float v = 0.f;
  for (int sl = 0; sl < slices; ++sl) v += ld_g(part + (int64_t)sl * total + i);
  st_g(phi + i, v);
}

template <int W>
static void launch_forest_explain(const ccfd_forest_explain_args& a, bool split, hipStream_t s) {
  const dim3 grid((unsigned)((a.n + 63) / 64), split ? (unsigned)a.slices : 1u);
  hipLaunchKernelGGL(forest_explain_kernel<W>, grid, dim3(kFrxThreads), 0, s, a, split ? 1 : (int)a.slices);
}

static bool frx_split(int64_t n, int slices) { return slices > 1 && (n + 63) / 64 < CCFD_FRX_SPLIT_BLOCKS; }

}  // namespace ccfd

extern "C" int64_t ccfd_forest_explain_workspace_bytes(int64_t n, int32_t slices) {
  if (n <= 0 || slices < 1 || slices > CCFD_FRX_MAX_SLICES) return 0;
  return ccfd::frx_split(n, slices) ? (int64_t)slices * n * ccfd::kF * 4 : 0;
}

extern "C" int ccfd_forest_explain_launch(const ccfd_forest_explain_args* a, void* stream) {
  using namespace ccfd;
  if (a == nullptr) { set_error("forest explain: null argument"); return -1; }
  if (a->paths < 0) { set_error("forest explain: paths < 0"); return -2; }
  if (a->width != 4 && a->width != 8 && a->width != 12 && a->width != 16) {
    set_error("forest explain: width is not 4, 8, 12 or 16");
    return -2;
  }
  if (a->slices < 1 || a->slices > CCFD_FRX_MAX_SLICES) { set_error("forest explain: slices outside 1..16"); return -2; }
  if (a->rec_words < 0 || a->rec_words > (1 << 30)) { set_error("forest explain: rec_words outside 0..2^30"); return -2; }
  if (a->n < 0) { set_error("forest explain: n < 0"); return -2; }
  if (a->n > (int64_t)0x7fffffff * 64) { set_error("forest explain: n too large for one launch"); return -2; }
  const int64_t need = (int64_t)kHeader + CCFD_FRX_RULE_BYTES + (int64_t)a->slices * kFrxWaves * 8 + (int64_t)a->rec_words * 4;
  if (a->blob_bytes < need) { set_error("forest explain: blob smaller than an FRX1 blob of this shape"); return -2; }
  if (a->n == 0) return 0;
  if (a->rows == nullptr || a->blob == nullptr || a->phi == nullptr) {
    set_error("forest explain: null argument");
    return -1;
  }
  if (reinterpret_cast<uintptr_t>(a->rows) & 15) { set_error("forest explain: G32 rows must be 16-byte aligned"); return -3; }
  if (reinterpret_cast<uintptr_t>(a->blob) & 15) { set_error("forest explain: the blob must be 16-byte aligned"); return -3; }
  const bool split = frx_split(a->n, a->slices);
  if (split && (a->workspace == nullptr || a->workspace_bytes < ccfd_forest_explain_workspace_bytes(a->n, a->slices))) {
    set_error("forest explain: workspace missing or smaller than ccfd_forest_explain_workspace_bytes(n, slices)");
    return -4;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  switch (a->width) {
    case 4: launch_forest_explain<4>(*a, split, s); break;
    case 8: launch_forest_explain<8>(*a, split, s); break;
    case 12: launch_forest_explain<12>(*a, split, s); break;
    default: launch_forest_explain<16>(*a, split, s); break;
  }
  if (split) {
    const int64_t total = a->n * kF;
    hipLaunchKernelGGL(forest_explain_sum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                       (const float*)a->workspace, a->phi, total, (int)a->slices);
  }
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
    set_error(std::string("forest explain: launch failed: ") + hipGetErrorString(e));
    return -5;
  }
  return 0;
}

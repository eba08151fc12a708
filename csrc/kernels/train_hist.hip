// Oblivious-GBDT training on G32 rows (train/trainer.py hist="hip"): the per-level gradient /
// hessian histograms and the per-tree update of raw scores, gradients and hessians.
//
// A G32 row's bytes 0..29 are exactly the trainer's bin matrix (bin = #borders < x), 32 B a
// row.  An oblivious tree's leaf is a pure function of those bytes and the splits chosen so
// far, so each thread recomputes it from the row it holds in registers: no leaf array, no
// expanded keys.
//
// Histogram kernel.  The level's histograms are [2^d][30][B] f32 twice (G and H): 15 KB at
// d = 0, B = 32 and 1.9 MB at d = 7, B = 64.  A workgroup privatises a FEATURE SLICE of them in
// LDS -- all 2^d leaves of `nf` consecutive features, sized to kHistLdsFloats (64 KiB, two
// workgroups a CU) -- so every (row, feature) costs two LDS float adds and nothing leaves the
// chip until the workgroup has summed all of its rows.  Levels whose histograms fit take one
// slice; the last levels take several (4 at d = 5, B = 32; 30 at d = 7, B = 64), each slice
// re-reading the rows (32 B a row against 2 x 4 B x nf of LDS adds).  `bps` workgroups share a
// slice, striding over the rows, and flush their non-zero cells with global float atomics:
// consecutive lanes flush consecutive bins of one (leaf, feature-run), i.e. contiguous 256-B
// wave requests.  The flush is at most (workgroups x LDS bytes) = 512 x 64 KiB = 32 MiB a
// level, ~25 us at the chip-wide float-atomic rate, whatever n is.
//
// Measured on 2 M rows, B = 32 (profiles/train_gbdt/): 0.63-0.67 ms a level at every depth,
// ~60x under two scatter_add passes.  What sets that time is the LDS float add itself: with the
// adds compiled out the kernel takes 0.03 ms (d = 0) to 0.11 ms (d = 5), with only the flush
// compiled out it takes the full time, and 256 workgroups take as long as 2048.  120 M
// ds_add_f32 lane-adds in ~0.6 ms is ~0.3 lane-adds a clock a CU, independent of how many
// cells the lanes spread over, so neither the slicing nor the flush is worth tuning before
// the accumulation stops being a float LDS atomic (docs/TUNING.md).
//
// Sums are f32 in arrival order (LDS adds inside a workgroup, global adds across them): the
// last bits can differ from run to run, as with scatter_add.
#include <algorithm>
#include <string>

#include "common.h"

namespace ccfd {

void set_error(const std::string& e);

constexpr int kHistThreads = 256;
constexpr int kHistLdsFloats = 16384;        // 64 KiB: G and H cells of one feature slice
constexpr int kHistRowsPerWg = 1024;         // fewer rows than this do not get their own workgroup
constexpr int kCuCount = 256;

struct G32Row { unsigned w[8]; };

__device__ __forceinline__ G32Row ld_g32_row(const uint8_t* __restrict__ rows, int64_t i) {
  const uint4 a = ld_g16(rows + i * CCFD_G32_ROW_BYTES);
  const uint4 b = ld_g16(rows + i * CCFD_G32_ROW_BYTES + 16);
  return G32Row{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}

// Byte f of the row, f a compile-time constant.
template <int kByte>
__device__ __forceinline__ unsigned g32_byte(const G32Row& r) {
  return (r.w[kByte >> 2] >> ((kByte & 3) * 8)) & 0xffu;
}

// leaf = sum_k (row[feat[k]] > bin[k]) << k for k < d.  The split features are wave-uniform
// but not compile-time constants: picking a byte out of the row's registers by such an index
// makes the compiler keep the row in scratch, so the d split bytes are read from memory
// instead -- byte loads that hit the cache line the row itself occupies.  feat / bin live in
// the kernarg segment and are read at constant indices (scalar loads).
template <int k = 0>
__device__ __forceinline__ unsigned g32_leaf(const uint8_t* __restrict__ row, const int32_t (&feat)[CCFD_GBDT_MAX_SPLITS],
                                             const int32_t (&bin)[CCFD_GBDT_MAX_SPLITS], int d) {
  unsigned leaf = 0;
  if (k < d) leaf = ((unsigned)ld_g(row + feat[k]) > (unsigned)bin[k] ? 1u : 0u) << k;
  if constexpr (k + 1 < CCFD_GBDT_MAX_SPLITS) leaf |= g32_leaf<k + 1>(row, feat, bin, d);
  return leaf;
}

__device__ __forceinline__ void lds_add(float* p, float v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <int kByte>
__device__ __forceinline__ void hist_feature(const G32Row& r, int f0, int f1, unsigned B, float* hg, float* hh,
                                             float g, float h) {
  if (kByte >= f0 && kByte < f1) {               // wave-uniform
    const unsigned b = g32_byte<kByte>(r);
    if (b < B) {                                 // a bin past the table: skipped, never out of bounds
      const unsigned c = (unsigned)(kByte - f0) * B + b;
      lds_add(hg + c, g);
      lds_add(hh + c, h);
    }
  }
  if constexpr (kByte + 1 < kF) hist_feature<kByte + 1>(r, f0, f1, B, hg, hh, g, h);
}

// Workgroup (slice, blk): features [slice * nf, min(30, slice * nf + nf)), rows blk * 256 + tid
// striding by bps * 256.  Dynamic LDS: 2 * 2^level * nf * n_bins floats.
__global__ __launch_bounds__(kHistThreads) void gbdt_hist_kernel(ccfd_gbdt_hist_args a, int nf, int bps) {
  extern __shared__ __attribute__((aligned(16))) float hs[];
  const int tid = threadIdx.x;
  const int slice = blockIdx.x / bps, blk = blockIdx.x % bps;
  const int f0 = slice * nf, f1 = min(kF, f0 + nf);
  const int B = a.n_bins, L = 1 << a.level;
  const int run = (f1 - f0) * B;                 // cells of one leaf in this slice
  const int cells = L * run;
  float* hg = hs;
  float* hh = hs + cells;
  for (int c = tid; c < 2 * cells; c += kHistThreads) hs[c] = 0.f;
  __syncthreads();

  const int64_t stride = (int64_t)bps * kHistThreads;
  for (int64_t i = (int64_t)blk * kHistThreads + tid; i < a.n; i += stride) {
    const G32Row r = ld_g32_row(a.rows, i);
    const float g = ld_g(a.grad + i), h = ld_g(a.hess + i);
    const unsigned off = g32_leaf(a.rows + i * CCFD_G32_ROW_BYTES, a.split_feat, a.split_bin, a.level) * (unsigned)run;
    hist_feature<0>(r, f0, f1, (unsigned)B, hg + off, hh + off, g, h);
  }
  __syncthreads();

  // cell c = (leaf, feature - f0, bin) -> G[(leaf * 30 + f0) * B + (c - leaf * run)]
  for (int c = tid; c < cells; c += kHistThreads) {
    const int leaf = c / run;
    const size_t o = ((size_t)leaf * kF + f0) * B + (c - leaf * run);
    const float g = hg[c], h = hh[c];
    if (g != 0.f) atomicAdd(a.G + o, g);
    if (h != 0.f) atomicAdd(a.H + o, h);
  }
}

__global__ __launch_bounds__(256) void gbdt_update_kernel(ccfd_gbdt_update_args a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const unsigned leaf = g32_leaf(a.rows + i * CCFD_G32_ROW_BYTES, a.split_feat, a.split_bin, a.depth);
  const float z = ld_g(a.raw + i) + ld_g(a.leaf_val + leaf);
  st_g(a.raw + i, z);
  if (a.grad != nullptr) {
    const float p = 1.f / (1.f + expf(-z));      // full-precision exp: the trainer's gradients
    st_g(a.grad + i, p - ld_g(a.y + i));
    st_g(a.hess + i, fmaxf(p * (1.f - p), 1e-6f));
  }
}

static bool splits_ok(const int32_t* feat, const int32_t* bin, int d) {
  for (int k = 0; k < d; ++k)
    if (feat[k] < 0 || feat[k] >= kF || bin[k] < 0 || bin[k] > 255) return false;
  return true;
}

}  // namespace ccfd

extern "C" int ccfd_gbdt_hist_launch(const ccfd_gbdt_hist_args* a, void* stream) {
  using namespace ccfd;
  if (a == nullptr || a->rows == nullptr || a->grad == nullptr || a->hess == nullptr || a->G == nullptr ||
      a->H == nullptr) {
    set_error("gbdt histogram: null argument");
    return -1;
  }
  if (a->level < 0 || a->level > CCFD_GBDT_HIST_MAX_LEVEL) { set_error("gbdt histogram: level outside 0..7"); return -2; }
  if (a->n_bins < 2 || a->n_bins > CCFD_GBDT_HIST_MAX_BINS) { set_error("gbdt histogram: n_bins outside 2..64"); return -2; }
  if (a->n < 1) { set_error("gbdt histogram: n < 1"); return -2; }
  if (!splits_ok(a->split_feat, a->split_bin, a->level)) {
    set_error("gbdt histogram: split feature outside 0..29 or split bin outside 0..255");
    return -2;
  }
  if (reinterpret_cast<uintptr_t>(a->rows) & 15) { set_error("gbdt histogram: G32 rows must be 16-byte aligned"); return -3; }
  const int L = 1 << a->level, B = a->n_bins;
  // feature slice: as many whole features (all leaves, G and H) as fit the LDS budget, then
  // evened out over the slices (30 features in 4 slices: 8 + 8 + 8 + 6)
  const int fit = kHistLdsFloats / (2 * L * B);            // >= 1 for every supported shape
  const int nslices = (kF + std::min(kF, fit) - 1) / std::min(kF, fit);
  const int nf = (kF + nslices - 1) / nslices;
  const size_t lds = (size_t)2 * L * nf * B * sizeof(float);
  // about one resident wave of workgroups: 2..8 a CU as the LDS footprint allows
  const int per_cu = (int)std::max<size_t>(2, std::min<size_t>(8, (160 * 1024) / lds));
  const int64_t by_rows = (a->n + kHistRowsPerWg - 1) / kHistRowsPerWg;
  const int bps = (int)std::max<int64_t>(1, std::min<int64_t>(by_rows, (kCuCount * per_cu) / nslices));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t out_bytes = (size_t)L * kF * B * sizeof(float);
  if (hipMemsetAsync(a->G, 0, out_bytes, s) != hipSuccess || hipMemsetAsync(a->H, 0, out_bytes, s) != hipSuccess) {
    set_error(std::string("gbdt histogram: memset failed: ") + hipGetErrorString(hipGetLastError()));
    return -5;
  }
  hipLaunchKernelGGL(gbdt_hist_kernel, dim3(nslices * bps), dim3(kHistThreads), lds, s, *a, nf, bps);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
    set_error(std::string("gbdt histogram: launch failed: ") + hipGetErrorString(e));
    return -5;
  }
  return 0;
}

extern "C" int ccfd_gbdt_update_launch(const ccfd_gbdt_update_args* a, void* stream) {
  using namespace ccfd;
  if (a == nullptr || a->rows == nullptr || a->leaf_val == nullptr || a->raw == nullptr) {
    set_error("gbdt update: null argument");
    return -1;
  }
  if ((a->grad == nullptr) != (a->hess == nullptr) || (a->grad != nullptr && a->y == nullptr)) {
    set_error("gbdt update: grad and hess go together and need y");
    return -1;
  }
  if (a->depth < 1 || a->depth > CCFD_GBDT_MAX_SPLITS) { set_error("gbdt update: depth outside 1..8"); return -2; }
  if (a->n < 1) { set_error("gbdt update: n < 1"); return -2; }
  if (a->n > (int64_t)0x7fffffff * 256) { set_error("gbdt update: n too large for one launch"); return -2; }
  if (!splits_ok(a->split_feat, a->split_bin, a->depth)) {
    set_error("gbdt update: split feature outside 0..29 or split bin outside 0..255");
    return -2;
  }
  if (reinterpret_cast<uintptr_t>(a->rows) & 15) { set_error("gbdt update: G32 rows must be 16-byte aligned"); return -3; }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(gbdt_update_kernel, dim3((unsigned)((a->n + 255) / 256)), dim3(256), 0, s, *a);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
    set_error(std::string("gbdt update: launch failed: ") + hipGetErrorString(e));
    return -5;
  }
  return 0;
}

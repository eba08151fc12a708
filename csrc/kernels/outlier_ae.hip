// Outlier scores of W64 rows: reconstruction error of an autoencoder 30 -> 64 -> L -> 64 -> 30
// (models/outlier.py holds the definition, the 'AEW1' blob layout, the numpy oracle
// wire_residuals / wire_scores and the lane-by-lane emulation; ops/kernels.py outlier_scores /
// OutlierMonitor).
//
// One wave works on 16-row tiles: lane (c = lane & 15, g = lane >> 4) loads chunk g of row c,
// one coalesced 1 KB request a tile, and that chunk IS the layer-1 B fragment (wire_operand,
// mlp_core.h).  The activations stay transposed, so every accumulator pair is the next MFMA's B
// operand after relu + bf16 pack, with no LDS round trip:
//   L1  4 M-tiles                h1 = bf16(relu(W1p x))            (b1 rides in K columns 30 / 31)
//   L2  2 M-tiles x 2 K-steps    z  = bf16(relu(b2 + W2 h1))       (latent zero-padded to 32)
//   L3  4 M-tiles                h3 = bf16(relu(b3 + W3 z))
//   L4  2 M-tiles x 2 K-steps    r  = b4 - T_hi x - T_lo x + W4 h3
// 20 mfma_f32_16x16x32_bf16 a tile.  The target T x comes from the same operand through a fixed
// matrix (stored negated), so it lands in the accumulator layout of W4 h3 and nothing is
// transposed: the residual of wire position 16t + 4g + j of row c sits in lane (c, g), tile t,
// register j.  Two tiles are scored per iteration: every weight fragment read from LDS (one
// ds_read_b128 a lane, 1 KB contiguous a wave: conflict-free) feeds two MFMAs, and the two
// dependency chains interleave.  The whole blob (21 KB) is staged in LDS once a workgroup.
//
// A row's result depends on nothing but its own operand column: not on n, the grid, its place
// in the tile or its neighbours (the matrix unit keeps B columns apart, and 0 * NaN in the T
// MFMAs spreads a non-finite feature over that row's 32 positions only).  No spin waits, no
// cross-workgroup dependencies, no persistent state: the kernel ends whatever the data holds.
// Counts are u32 LDS adds per workgroup, flushed with 64-bit global atomic adds.
#include <algorithm>
#include <string>

#include "mlp_core.h"

namespace ccfd {

void set_error(const std::string& e);

constexpr int kAeThreads = 256;
constexpr int kAeWaves = kAeThreads / 64;
constexpr int kAeRowsPerWg = kAeWaves * 2 * kTileRows;    // one pair of tiles a wave: 128 rows
constexpr int kAeBlob = CCFD_OUT_BLOB_BYTES;
constexpr int kAeOffW1 = kOffNorm + 256;                  // models/outlier.py OFF_*
constexpr int kAeOffW2 = kAeOffW1 + 4 * 64 * 16;
constexpr int kAeOffW3 = kAeOffW2 + 4 * 64 * 16;
constexpr int kAeOffW4 = kAeOffW3 + 4 * 64 * 16;
constexpr int kAeOffTH = kAeOffW4 + 4 * 64 * 16;
constexpr int kAeOffTL = kAeOffTH + 2 * 64 * 16;
constexpr int kAeOffB2 = kAeOffTL + 2 * 64 * 16;
constexpr int kAeOffB3 = kAeOffB2 + 2 * 64;
constexpr int kAeOffB4 = kAeOffB3 + 4 * 64;
static_assert(kAeOffB4 + 2 * 64 == kAeBlob, "blob layout");
constexpr unsigned kAeMagic = 0x31574541u;                // 'AEW1'

__device__ __forceinline__ bf16x8 ae_pair(const f32x4& a, const f32x4& b) {
  return __builtin_bit_cast(bf16x8, make_uint4(relu_pack_bf16x2(a[0], a[1]), relu_pack_bf16x2(a[2], a[3]),
                                               relu_pack_bf16x2(b[0], b[1]), relu_pack_bf16x2(b[2], b[3])));
}

__device__ __forceinline__ f32x4 ae_mfma(const bf16x8& a, const bf16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// Either bf16 half of w is inf or NaN.
__device__ __forceinline__ bool ae_bad2(unsigned w) {
  return (w & 0x7f800000u) == 0x7f800000u || (w & 0x7f80u) == 0x7f80u;
}

// The layer-1 operand of a lane chunk.  A chunk with a non-finite feature gets a NaN in its
// first two slots: wire_operand clamps Amount before the log, which would hide a NaN or -inf
// Amount, and an inf alone could leave +-inf, not NaN, in the residual of its own position.
__device__ __forceinline__ bf16x8 ae_operand(const WireRegs& r, bool g3, const MlpWireLane& L) {
  const bf16x8 x = wire_operand(r, g3, L);
  const bool tail = g3 ? ((r.v.z & 0x7f800000u) == 0x7f800000u) || ((r.v.w & 0x7f800000u) == 0x7f800000u)
                       : ae_bad2(r.v.z) || ae_bad2(r.v.w);
  const bool bad = ae_bad2(r.v.x) || ae_bad2(r.v.y) || tail;
  uint4 u = __builtin_bit_cast(uint4, x);
  u.x = bad ? 0x7fc07fc0u : u.x;
  return __builtin_bit_cast(bf16x8, u);
}

// Residuals of two tiles: ra / rb [t] = accumulator of M-tile t of layer 4.
__device__ __forceinline__ void ae_tile_x2(const char* sblob, const bf16x8& xa, const bf16x8& xb, int g, int lane,
                                           f32x4 ra[2], f32x4 rb[2]) {
  const bf16x8* W1f = reinterpret_cast<const bf16x8*>(sblob + kAeOffW1);
  const bf16x8* W2f = reinterpret_cast<const bf16x8*>(sblob + kAeOffW2);
  const bf16x8* W3f = reinterpret_cast<const bf16x8*>(sblob + kAeOffW3);
  const bf16x8* W4f = reinterpret_cast<const bf16x8*>(sblob + kAeOffW4);
  const bf16x8* THf = reinterpret_cast<const bf16x8*>(sblob + kAeOffTH);
  const bf16x8* TLf = reinterpret_cast<const bf16x8*>(sblob + kAeOffTL);
  const f32x4* b2q = reinterpret_cast<const f32x4*>(sblob + kAeOffB2);
  const f32x4* b3q = reinterpret_cast<const f32x4*>(sblob + kAeOffB3);
  const f32x4* b4q = reinterpret_cast<const f32x4*>(sblob + kAeOffB4);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  // layer 4's accumulators start as b4 - T_hi x - T_lo x: independent of the chain, issued first
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const f32x4 b4 = b4q[u * 4 + g];
    const bf16x8 th = THf[u * 64 + lane], tl = TLf[u * 64 + lane];
    ra[u] = ae_mfma(tl, xa, ae_mfma(th, xa, b4));
    rb[u] = ae_mfma(tl, xb, ae_mfma(th, xb, b4));
  }
  // layer 1: M-tiles (2s, 2s+1) are K-step s of layer 2
  bf16x8 ha[2], hb[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const bf16x8 w0 = W1f[(2 * s) * 64 + lane], w1 = W1f[(2 * s + 1) * 64 + lane];
    const f32x4 a0 = ae_mfma(w0, xa, zero), b0 = ae_mfma(w0, xb, zero);
    const f32x4 a1 = ae_mfma(w1, xa, zero), b1 = ae_mfma(w1, xb, zero);
    ha[s] = ae_pair(a0, a1);
    hb[s] = ae_pair(b0, b1);
  }
  // layer 2: its two M-tiles are the single K-step of layer 3
  f32x4 a2[2], b2[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    f32x4 aa = b2q[u * 4 + g], bb = aa;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const bf16x8 w = W2f[(u * 2 + s) * 64 + lane];
      aa = ae_mfma(w, ha[s], aa);
      bb = ae_mfma(w, hb[s], bb);
    }
    a2[u] = aa;
    b2[u] = bb;
  }
  const bf16x8 za = ae_pair(a2[0], a2[1]), zb = ae_pair(b2[0], b2[1]);
  // layer 3
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const bf16x8 w0 = W3f[(2 * s) * 64 + lane], w1 = W3f[(2 * s + 1) * 64 + lane];
    const f32x4 c0 = b3q[(2 * s) * 4 + g], c1 = b3q[(2 * s + 1) * 4 + g];
    const f32x4 a0 = ae_mfma(w0, za, c0), b0 = ae_mfma(w0, zb, c0);
    const f32x4 a1 = ae_mfma(w1, za, c1), b1 = ae_mfma(w1, zb, c1);
    ha[s] = ae_pair(a0, a1);
    hb[s] = ae_pair(b0, b1);
  }
  // layer 4
#pragma unroll
  for (int u = 0; u < 2; ++u) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const bf16x8 w = W4f[(u * 2 + s) * 64 + lane];
      ra[u] = ae_mfma(w, ha[s], ra[u]);
      rb[u] = ae_mfma(w, hb[s], rb[u]);
    }
  }
}

struct AeCountsLds {
  unsigned v[CCFD_OUTLIER_SLOTS];
};

__device__ __forceinline__ void ae_lds_add(unsigned* p, unsigned v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Score, store and count one tile: r[t][j] = residual of wire position 16t + 4g + j of row c.
__device__ __forceinline__ void ae_finish(const ccfd_outlier_args& a, const f32x4 r[2], int64_t row, bool valid,
                                          int g, float threshold, AeCountsLds* cnt) {
  // the lane's 8 squares in a fixed order, no fused multiply-add (the compiler contracts a * b + c
  // by default, also through the _rn intrinsics: plain operators under the pragma), then the two cross-group adds: float add commutes,
  // so all four lane groups end with the same bits
#pragma clang fp contract(off)
  float q = r[0][0] * r[0][0];
#pragma unroll
  for (int j = 1; j < 4; ++j) q = q + r[0][j] * r[0][j];
#pragma unroll
  for (int j = 0; j < 4; ++j) q = q + r[1][j] * r[1][j];
  q = q + __shfl_xor(q, 16);
  q = q + __shfl_xor(q, 32);
  const float score = q * (1.0f / 30.0f);
  if (valid) {
    if (g == 0) st_g(a.score + row, score);
    if (a.resid_out != nullptr) {
      f32x4* out = reinterpret_cast<f32x4*>(a.resid_out + row * 32 + 4 * g);
      st_g(out, r[0]);
      st_g(out + 4, r[1]);
    }
  }
  if (cnt == nullptr) return;
  const unsigned bits = __float_as_uint(score);
  const bool finite = (bits & 0x7f800000u) != 0x7f800000u;
  const bool flagged = valid && score > threshold;             // NaN: false
  if (valid && g == 0) {
    if (finite) {
      const int cell = min(max((int)((bits >> 23) & 255u) - 111, 0), 31);
      ae_lds_add(&cnt->v[CCFD_OUT_HIST + cell], 1u);
    } else {
      ae_lds_add(&cnt->v[CCFD_OUT_INVALID], 1u);
    }
    if (flagged) ae_lds_add(&cnt->v[CCFD_OUT_FLAGGED], 1u);
  }
  if (__ballot(flagged) == 0ull) return;                       // wave-uniform: flagged rows are rare
  // largest squared residual of the row, lowest wire position on a tie; positions 30 / 31 are no features
  float best = -1.f;
  int pos = 0;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = 16 * t + 4 * g + j;
      const float s = r[t][j] * r[t][j];
      if (p < kF && s > best) { best = s; pos = p; }
    }
  }
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const float ob = __shfl_xor(best, o);
    const int op = __shfl_xor(pos, o);
    if (ob > best || (ob == best && op < pos)) { best = ob; pos = op; }
  }
  if (flagged && g == 0) {
    // wire position -> canonical feature: V1..V28 are 1..28, Time 0, Amount 29
    const int feat = pos < 28 ? pos + 1 : (pos == 28 ? 0 : kAmountCol);
    ae_lds_add(&cnt->v[CCFD_OUT_TOP + feat], 1u);
  }
}

__global__ __launch_bounds__(kAeThreads) void outlier_ae_kernel(ccfd_outlier_args a) {
  __shared__ __attribute__((aligned(16))) char sblob[kAeBlob];
  __shared__ AeCountsLds cnt;
  const int tid = threadIdx.x;
  mlp_stage(a.blob, sblob, tid, kAeThreads, kAeBlob);
  for (int i = tid; i < CCFD_OUTLIER_SLOTS; i += kAeThreads) cnt.v[i] = 0u;
  __syncthreads();

  const int lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const MlpWireLane L = mlp_wire_lane(sblob);
  const float threshold = (a.flags & CCFD_OUT_FLAG_THRESHOLD) ? a.threshold : *reinterpret_cast<const float*>(sblob + 12);
  AeCountsLds* cp = a.counts != nullptr ? &cnt : nullptr;

  const int64_t n = a.n;
  const int64_t pairs = (n + 2 * kTileRows - 1) / (2 * kTileRows);
  const int64_t stride = (int64_t)gridDim.x * kAeWaves;
  unsigned counted = 0;
  for (int64_t p = (int64_t)blockIdx.x * kAeWaves + wave; p < pairs; p += stride) {
    const int64_t row0 = p * (2 * kTileRows) + c, row1 = row0 + kTileRows;
    const bool v0 = row0 < n, v1 = row1 < n;
    WireRegs r0, r1;
    r0.v = v0 ? ld_g16(a.rows + row0 * CCFD_WIRE_ROW_BYTES + 16 * g) : make_uint4(0u, 0u, 0u, 0u);
    r1.v = v1 ? ld_g16(a.rows + row1 * CCFD_WIRE_ROW_BYTES + 16 * g) : make_uint4(0u, 0u, 0u, 0u);
    const bf16x8 xa = ae_operand(r0, g == 3, L), xb = ae_operand(r1, g == 3, L);
    f32x4 ra[2], rb[2];
    ae_tile_x2(sblob, xa, xb, g, lane, ra, rb);
    ae_finish(a, ra, row0, v0, g, threshold, cp);
    ae_finish(a, rb, row1, v1, g, threshold, cp);
    counted += (unsigned)(v0 && g == 0) + (unsigned)(v1 && g == 0);
  }
  if (cp != nullptr) {
    if (counted) ae_lds_add(&cnt.v[CCFD_OUT_ROWS], counted);
    __syncthreads();
    for (int i = tid; i < CCFD_OUTLIER_SLOTS; i += kAeThreads) {
      const unsigned v = cnt.v[i];
      if (v) atomicAdd(a.counts + i, (unsigned long long)v);
    }
  }
}

}  // namespace ccfd

extern "C" int ccfd_outlier_ae_launch(const ccfd_outlier_args* a, void* stream) {
  using namespace ccfd;
  if (a == nullptr || a->blob == nullptr || ((a->rows == nullptr || a->score == nullptr) && a->n != 0)) {
    set_error("outlier scores: null argument");
    return -1;
  }
  if (a->n < 0) { set_error("outlier scores: n < 0"); return -2; }
  if (a->max_workgroups < 1) { set_error("outlier scores: max_workgroups < 1"); return -2; }
  if (reinterpret_cast<uintptr_t>(a->rows) & 15) {
    set_error("outlier scores: W64 rows must be 16-byte aligned");
    return -3;
  }
  if ((reinterpret_cast<uintptr_t>(a->blob) & 15) || (reinterpret_cast<uintptr_t>(a->resid_out) & 15) ||
      (reinterpret_cast<uintptr_t>(a->score) & 3) || (reinterpret_cast<uintptr_t>(a->counts) & 7)) {
    set_error("outlier scores: blob and resid_out must be 16-byte, counts 8-byte and score 4-byte aligned");
    return -3;
  }
  if (a->blob_bytes != kAeBlob || (unsigned)a->magic != kAeMagic || a->latent < 1 || a->latent > 32) {
    set_error("outlier scores: not an 'AEW1' blob of " + std::to_string(kAeBlob) + " bytes with a latent of 1..32");
    return -4;
  }
  if (a->n == 0) return 0;
  const int64_t by_rows = (a->n + kAeRowsPerWg - 1) / kAeRowsPerWg;
  const int grid = (int)std::min<int64_t>(a->max_workgroups, by_rows);
  // a workgroup's cells are u32: it must see fewer than 2^32 rows
  if ((a->n + grid - 1) / grid + kAeRowsPerWg > (int64_t)0xffffffffll) {
    set_error("outlier scores: more than 2^32 rows a workgroup; raise max_workgroups or split the launch");
    return -2;
  }
  hipLaunchKernelGGL(outlier_ae_kernel, dim3(grid), dim3(kAeThreads), 0, reinterpret_cast<hipStream_t>(stream), *a);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
    set_error(std::string("outlier scores: launch failed: ") + hipGetErrorString(e));
    return -5;
  }
  return 0;
}

// Sampled Shapley values of the MLP on W64 rows against one baseline row, in logit space
// (permutation sampling in antithetic pairs; the definition is in docs/EXPLAIN.md and
// models/explain_mlp.py, whose shapley_mlp_table is the oracle and whose MlpExplainTable.pack
// writes the 'MLX1' table read here).
//
// One row per wave; the 4 waves of a workgroup stride over the rows and share the wire blob and
// the table, staged in LDS once.  A permutation is 32 coalition rows -- slot s carries the row's
// bits on the first s positions of the permutation and the baseline's elsewhere (slots 30 and 31
// are both the full row) -- i.e. two 16-row tiles through mlp_logit_w64_x2.  Lane (g, c) holds
// the 16-byte chunk 16g of the row and of the baseline and builds its chunk of slots c and
// 16 + c by bit-select from the slot's mask word: chunks 0..2 are eight 16-bit positions,
// chunk 3 is four 16-bit positions plus the Time and Amount dwords.  The logit of slot l then
// sits in lane l < 32 (every lane group holds its tile's 16 logits), d[k] = z[k+1] - z[k] comes
// from one shuffle, and lane j < 30 adds d[inv[p][j]], the step at which position j joined, to
// its own register.  No atomics; the sum over p runs in ascending order and depends on neither
// n, the grid nor the other rows, so a row explained alone gets the bits it gets in a batch.
#include <algorithm>
#include <string>

#include "mlp_core.h"

namespace ccfd {

void set_error(const std::string& e);

constexpr int kMlxThreads = 256;
constexpr int kMlxWaves = kMlxThreads / 64;
constexpr int kMlxSlots = 32;
constexpr int kMlxHead = 2 * kHeader;                       // header + the baseline row
constexpr unsigned kMlxMagic = 0x31584c4du;                 // 'MLX1'

constexpr int64_t mlx_table_bytes(int perms) { return kMlxHead + (int64_t)perms * (4 + 1) * kMlxSlots; }

// the slot's 16-byte chunk: bit (lo[d] / hi[d]) of the mask word selects the row's low / high
// half of dword d, else the baseline's
__device__ __forceinline__ WireRegs mlx_select(const uint4& x, const uint4& b, unsigned m, const unsigned (&lo)[4],
                                               const unsigned (&hi)[4]) {
  const unsigned xs[4] = {x.x, x.y, x.z, x.w}, bs[4] = {b.x, b.y, b.z, b.w};
  unsigned o[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const unsigned sel = ((0u - ((m >> lo[d]) & 1u)) & 0x0000ffffu) | ((0u - ((m >> hi[d]) & 1u)) & 0xffff0000u);
    o[d] = (xs[d] & sel) | (bs[d] & ~sel);
  }
  WireRegs r;
  r.v = make_uint4(o[0], o[1], o[2], o[3]);
  return r;
}

// 2 waves a SIMD: the compiler keeps every weight fragment of the chain in VGPRs across the
// permutation loop (211 VGPRs, no scratch), so the loop reads LDS for the masks alone.  Asked for
// 3 or 4 waves it still hoists the fragments and spills them (208 / 600 bytes of scratch a lane;
// 4 waves measured 6.8 times slower).
__global__ __launch_bounds__(kMlxThreads) __attribute__((amdgpu_waves_per_eu(2)))
void mlp_explain_kernel(ccfd_mlp_explain_args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sblob = smem;                                       // kMlpBlobWire bytes
  char* stab = smem + kMlpBlobWire;                         // the MLX1 table
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int P = a.perms;

  mlp_stage(a.blob, sblob, tid, kMlxThreads, kMlpBlobWire);
  mlp_stage(a.table, stab, tid, kMlxThreads, (int)mlx_table_bytes(P));
  __syncthreads();

  const MlpWireLane L = mlp_wire_lane(sblob);
  const uint4 base = *reinterpret_cast<const uint4*>(stab + kHeader + 16 * g);
  const unsigned* masks = reinterpret_cast<const unsigned*>(stab + kMlxHead);
  const unsigned char* inv = reinterpret_cast<const unsigned char*>(stab + kMlxHead + 4 * kMlxSlots * P);
  unsigned lo[4], hi[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    lo[d] = 8u * g + 2u * d;
    hi[d] = lo[d] + 1u;
  }
  if (g == 3) { lo[2] = hi[2] = 28u; lo[3] = hi[3] = 29u; }  // Time, Amount: whole dwords
  // wire position j -> canonical feature (contracts/transaction.py WIRE_PERM)
  const int feat = lane < 28 ? lane + 1 : lane == 28 ? 0 : kAmountCol;
  const float inv_p = (float)P;

  for (int64_t row = (int64_t)blockIdx.x * kMlxWaves + wave; row < a.n; row += (int64_t)gridDim.x * kMlxWaves) {
    const uint4 x = ld_g16(a.rows + row * CCFD_WIRE_ROW_BYTES + 16 * g);
    float acc = 0.f;
    for (int p = 0; p < P; ++p) {
      const unsigned m0 = masks[p * kMlxSlots + c], m1 = masks[p * kMlxSlots + 16 + c];
      const WireRegs r0 = mlx_select(x, base, m0, lo, hi), r1 = mlx_select(x, base, m1, lo, hi);
      float z0, z1;
      mlp_logit_w64_x2(sblob, L, r0, r1, g, lane, z0, z1);
      const float zl = (lane & 16) ? z1 : z0;               // lane l < 32: the logit of slot l
      const float d = __shfl(zl, (lane + 1) & 31) - zl;     // lane k < 31: d[k]
      const int at = inv[p * kMlxSlots + (lane & 31)];
      acc += __shfl(d, at & 31);
      if (a.z_out != nullptr && lane < kMlxSlots) st_g(a.z_out + ((row * P + p) * kMlxSlots + lane), zl);
    }
    if (lane < kF) st_g(a.phi + row * kF + feat, acc / inv_p);
  }
}

}  // namespace ccfd

extern "C" int ccfd_mlp_explain_launch(const ccfd_mlp_explain_args* a, void* stream) {
  using namespace ccfd;
  if (a == nullptr) { set_error("mlp explain: null argument"); return -1; }
  if (a->n < 0) { set_error("mlp explain: n < 0"); return -2; }
  if (a->n > (int64_t)0x7fffffff) { set_error("mlp explain: n too large for one launch"); return -2; }
  if (a->perms < 2 || a->perms > CCFD_MLX_MAX_PERMS || (a->perms & 1)) {
    set_error("mlp explain: perms must be even, 2..256");
    return -2;
  }
  if (a->max_workgroups < 1) { set_error("mlp explain: max_workgroups < 1"); return -2; }
  if (a->table_head[0] != kMlxMagic) { set_error("mlp explain: the table is not an MLX1 table"); return -2; }
  if (a->table_head[1] != (uint32_t)a->perms) { set_error("mlp explain: the table's P differs from perms"); return -2; }
  if (a->table_bytes != mlx_table_bytes(a->perms)) {
    set_error("mlp explain: table_bytes is not the MLX1 size of this many permutations");
    return -2;
  }
  if (a->blob_bytes != kMlpBlobWire) { set_error("mlp explain: the blob is not a W64 wire MLP blob"); return -2; }
  if (a->n == 0) return 0;
  if (a->rows == nullptr || a->blob == nullptr || a->table == nullptr || a->phi == nullptr) {
    set_error("mlp explain: null argument");
    return -1;
  }
  if (reinterpret_cast<uintptr_t>(a->rows) & 15) { set_error("mlp explain: W64 rows must be 16-byte aligned"); return -3; }
  if ((reinterpret_cast<uintptr_t>(a->blob) | reinterpret_cast<uintptr_t>(a->table)) & 15) {
    set_error("mlp explain: the blob and the table must be 16-byte aligned");
    return -3;
  }
  const int64_t groups = std::min<int64_t>(a->max_workgroups, (a->n + kMlxWaves - 1) / kMlxWaves);
  const size_t lds = (size_t)kMlpBlobWire + (size_t)mlx_table_bytes(a->perms);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mlp_explain_kernel, dim3((unsigned)groups), dim3(kMlxThreads), lds, s, *a);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
    set_error(std::string("mlp explain: launch failed: ") + hipGetErrorString(e));
    return -5;
  }
  return 0;
}

// What the two general-tree kernels share: score_forest.hip (f32 rows, blob 'FRS1') and
// score_forest_bins.hip (G32 / G20 rows, blob 'FRB1') -- the node word and the limits of the
// node table, the device view of a blob (fr_view), the staging of the node table
// (fr_stage_nodes), the walk itself (fr_walk / fr_tail / fr_sum, over a kernel's own row
// policy), and on the host the cache of blob headers and the preparation of a launch
// (forest_prepare, fr_lds_opt_in).  models/forest.py describes both blobs.
#pragma once

#include "common.h"

namespace ccfd {

// Node-table LDS budget (mirrored by models/forest.py LDS_NODE_BYTES).  Static LDS of the f32
// kernel is ~8.9 KB (xs 7.5 KB + part 1 KB + epilogue), a CU has 160 KiB: tables up to
// ~71 KB leave room for two workgroups per CU, anything larger for one.  One workgroup per CU
// is one wave per SIMD, which is why the walk carries several chains per lane; an LDS gather at
// that occupancy still beats an L2 gather (~10x the latency) at full occupancy, so the
// budget is everything one workgroup can take: 144 KiB = 18432 nodes (a 100 x depth-6
// complete ensemble is 12700).  Smaller tables allocate only what they need and keep the
// higher occupancy.
constexpr int kNodeLdsBytes = 144 * 1024;
constexpr int kFrMaxDepth = 64;
constexpr int kFrMaxNodes = 1 << 24;          // child index field: 24 bits

// w: bits 0..4 feature, bit 5 leaf, bits 8..31 left child.  v: the threshold of an inner node
// (FRS1: f32; FRB1: its bin index as u32 bits), the f32 value of a leaf.
struct FrNode { unsigned w; float v; };

// Node i as one 64-bit word: w in the low half, v in the high half.
template <bool kLds>
__device__ __forceinline__ FrNode fr_node(const uint2* __restrict__ gn, const uint2* ln, unsigned i) {
  unsigned long long q;
  if constexpr (kLds) q = reinterpret_cast<const unsigned long long*>(ln)[i];
  else q = *(const CCFD_GAS unsigned long long*)(gn + i);
  return FrNode{(unsigned)q, __uint_as_float((unsigned)(q >> 32))};
}

// A blob as the kernels read it: the link (sig: sigmoid, otherwise identity clamped to [0, 1]),
// T, n_nodes, base and (FRB1) the bin table's stamp from its own 64-byte header, so what bounds
// every read is the blob itself; then the {root, depth} pair of every tree, and the node table.
struct FrView {
  bool sig; int T, n_nodes; float base; unsigned stamp;
  const int* __restrict__ tree; const uint2* __restrict__ gn;
};

__device__ __forceinline__ FrView fr_view(const void* blob_) {
  const char* blob = reinterpret_cast<const char*>(blob_);
  const int* __restrict__ hdr = reinterpret_cast<const int*>(blob);
  const int T = hdr[2];
  return FrView{(hdr[1] & 1) != 0, T, hdr[5], gbb_base(blob), (unsigned)hdr[6],
                reinterpret_cast<const int*>(blob + kHeader),
                reinterpret_cast<const uint2*>(blob + kHeader + ((8 * (size_t)T + 15) & ~(size_t)15))};
}

// The node table into LDS, by the whole workgroup of kThreads.  16-byte copies: the node section
// is padded to 16 B, and so is its LDS.  Eight loads are in flight per thread before the first
// store, where a load-wait-store loop pays one L2 round trip per 4 KB of table; a 65536-row
// micro-batch is one chunk per wave, so the staging is a visible part of its launch.
template <int kThreads>
__device__ __forceinline__ void fr_stage_nodes(const uint2* __restrict__ gn, uint2* nl, int n_nodes, int tid) {
  constexpr int kInFlight = 8;
  const uint4* s4 = reinterpret_cast<const uint4*>(gn);
  uint4* d4 = reinterpret_cast<uint4*>(nl);
  const int n16 = (n_nodes + 1) / 2;
  for (int i0 = tid; i0 < n16; i0 += kThreads * kInFlight) {
    uint4 v[kInFlight];
#pragma unroll
    for (int k = 0; k < kInFlight; ++k)
      if (i0 + kThreads * k < n16) v[k] = ld_g16(s4 + i0 + kThreads * k);
#pragma unroll
    for (int k = 0; k < kInFlight; ++k)
      if (i0 + kThreads * k < n16) d4[i0 + kThreads * k] = v[k];
  }
}

// Walk U trees (t0, t0 + kStride, ...) for the lane's row; returns the leaf sum.  One step is
//   next = child + (!leaf && row goes right)
// `Row` is the kernel's view of the lane's row: fetch(w) reads the operand of node word w, and
// right(x, node) says whether that operand sends the row right.  All U fetches are issued
// before the first compare.  The step is branch-free on purpose: a leaf's child field is its
// own index and its feature field is 0, so a finished lane stays put, its (ignored) operand
// read is in bounds, and the U chains' loads stay interleaved -- a short-circuit `&&` here
// compiles to one exec-masked branch per chain, each waiting for its own LDS read.
template <int U, bool kLds, int kStride, class Row>
__device__ __forceinline__ float fr_walk(const int* __restrict__ tree, const uint2* __restrict__ gn, const uint2* ln,
                                         const Row& row, int t0) {
  FrNode nd[U];
  int depth = 0;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int t = t0 + kStride * u;
    const unsigned root = (unsigned)__builtin_amdgcn_readfirstlane(tree[2 * t]);
    depth = max(depth, __builtin_amdgcn_readfirstlane(tree[2 * t + 1]));
    nd[u] = fr_node<kLds>(gn, ln, root);
  }
  for (int s = 0; s < depth; ++s) {
    decltype(row.fetch(0u)) x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) x[u] = row.fetch(nd[u].w);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned inner = ((nd[u].w >> 5) & 1u) ^ 1u;
      const unsigned gt = row.right(x[u], nd[u]) ? 1u : 0u;
      nd[u] = fr_node<kLds>(gn, ln, (nd[u].w >> 8) + (gt & inner));
    }
  }
  float acc = 0.f;
#pragma unroll
  for (int u = 0; u < U; ++u) acc += nd[u].v;
  return acc;
}

// One group of U trees if that many are left, then the smaller groups: the tail in halving
// group sizes (a single-tree walk costs the latency of a full group).
template <int U, bool kLds, int kStride, class Row>
__device__ __forceinline__ void fr_tail(const int* __restrict__ tree, const uint2* __restrict__ gn, const uint2* ln,
                                        const Row& row, int T, int& t, float& acc) {
  if (t + kStride * (U - 1) + 1 <= T) { acc += fr_walk<U, kLds, kStride>(tree, gn, ln, row, t); t += kStride * U; }
  if constexpr (U > 1) fr_tail<U / 2, kLds, kStride>(tree, gn, ln, row, T, t, acc);
}

// The trees t0, t0 + kStride, ... below T, kU at a time, then the tail.  Order of the float
// additions: the leaves of a group from u = 0, the groups in tree order.  "A group of U is left"
// is spelled `last tree + 1 <= T`: with `last tree < T` the binned kernel's group loop compiles
// to code 3 % slower on an LDS table (profiles/forest_core/README.md).
template <int kU, bool kLds, int kStride, class Row>
__device__ __forceinline__ float fr_sum(const FrView& m, const uint2* ln, const Row& row, int t0) {
  static_assert((kU & (kU - 1)) == 0, "group sizes halve down to 1");
  float acc = 0.f;
  int t = t0;
  for (; t + kStride * (kU - 1) + 1 <= m.T; t += kStride * kU) acc += fr_walk<kU, kLds, kStride>(m.tree, m.gn, ln, row, t);
  if constexpr (kU > 1) fr_tail<kU / 2, kLds, kStride>(m.tree, m.gn, ln, row, m.T, t, acc);
  return acc;
}

// A launch needs the node count (LDS size) and re-checks the shape, both from the blob's
// header, which lives in device memory: it is read once per blob address and cached;
// ccfd_forest_blob_changed() drops an address whose memory was rewritten (ops/kernels.py
// calls it for every blob it uploads).  A stale entry cannot make a kernel read out of
// bounds -- the kernels take T / n_nodes from the device header and compare n_nodes with
// the LDS they were given -- it only costs the table its LDS residency.
// The read is a blocking copy, so the first launch with a blob cannot sit inside a stream capture.
struct FrHeader { char magic[4]; int flags, T, depth; float base; int n_nodes; int stamp; int pad[9]; };
static_assert(sizeof(FrHeader) == kHeader, "FRS1 / FRB1 header is 64 bytes");

int forest_header(const void* blob, FrHeader& h);    // 0, or -1 if the header cannot be read

// The shape checks of both launches; on refusal the message is set and the result is false.
bool forest_shape_ok(const FrHeader& h, const ccfd_score_args& a);

// What both launches do first (score_forest.hip): read the header, refuse a blob whose magic is
// not `magic` (with `other_hint` if it is `other`, the other kernel's), check the shape, size the
// node table's LDS (lds_nodes; 0: walked from global memory) and the workgroups a CU holds beside
// the kernel's own `fixed_lds` bytes (<= 4: 16 waves / CU).  0, or the launch's return code.
struct FrLaunch { FrHeader h; int lds_nodes, per_cu; };
int forest_prepare(const ccfd_score_args& a, const char* magic, const char* other, const char* other_hint,
                   int fixed_lds, FrLaunch& p);

// Dynamic LDS past 64 KB needs an opt-in, once per kernel; the launch itself reports a refusal.
template <class Kernel>
inline void fr_lds_opt_in(Kernel kernel, int bytes) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  (void)hipGetLastError();
}

}  // namespace ccfd

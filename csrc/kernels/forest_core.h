// What the two general-tree kernels share: score_forest.hip (f32 rows, blob 'FRS1') and
// score_forest_bins.hip (G32 / G20 rows, blob 'FRB1') -- the node word, the limits of the node
// table, and the host-side cache of blob headers (models/forest.py describes both blobs).
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

}  // namespace ccfd

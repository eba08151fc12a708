// G32 / G20 oblivious-GBDT scorer, persistent variant (engine exec_mode = 1; protocol in
// persist_core.h; row format and level form in g32_core.h).  The leaf tables
// are staged into LDS ONCE per resident workgroup (a launch per micro-batch re-stages them
// in every workgroup), and a claimed item is 4 waves x `cpw` 64-row chunks, the next chunk
// of a wave in flight while the current one is evaluated.
//
// Measured against it in round 6 (config 4, depth 4; profiles/r6/pass_c, pass_d; the code is
// in commit 95a7cf0): both chunks of a wave walked through the trees as a pair (R = 2: two
// row chains a lane) 2.540 vs 2.545e9 tx/s -- the tree walk's ILP is not the limit; a
// wave-specialised workgroup (a loader wave filling LDS item stages, 4 scorer waves reading
// only LDS) 1.78-2.05e9 in every variant (claim-ahead, two loaders, double-buffered without
// claim-ahead): queued items raise the micro-batch latency, and at a fixed ring depth the
// rate falls with it (Little's law: 4 x 65536 rows / batch latency).
#include <cstdio>
#include <vector>

#include "g32_core.h"
#include "persist_core.h"

namespace ccfd {

#ifdef CCFD_EXP_ITEM_TRACE
// Experiment build only (scripts/build_ab.py -D CCFD_EXP_ITEM_TRACE; never in the default
// library): thread 0 stamps each claimed item's phases -- claim atomic, wait for the posting +
// descriptor, first chunk's load, scoring, release + ticket -- into a device ring that the
// engine dumps at teardown (engine.cpp persist_free; bench/experiments/item_trace.py reads it).
struct ItemTrace {
  unsigned long long item, wg, t_claim, t_claimed, t_seen, t_desc, t_load, t_scored, t_done;
};
constexpr unsigned kItemTraceCap = 1u << 17;
__device__ ItemTrace g_item_trace[kItemTraceCap];
__device__ unsigned long long g_item_trace_n;
#define CCFD_ITRACE(stmt) stmt
#else
#define CCFD_ITRACE(stmt)
#endif

// kW waves per workgroup: 4 (default), or 8 in an experiment build (CCFD_EXP_G20_WAVES8: two
// waves per SIMD, each scoring half as many chunks of an item, so one wave's tree-walk
// latency hides behind the other's)
template <int D, bool kR, bool kGL, bool kG20, int kW = kG32Waves>
__global__ __launch_bounds__(64 * kW) void persist_gbdt_g32_kernel(ccfd_persist_args a) {
  extern __shared__ __attribute__((aligned(16))) float lv[];   // T * L floats
  __shared__ uint4 xt[kW][128];
  __shared__ EpilogueLds epi;
  __shared__ ccfd_persist_desc sdesc;
  __shared__ unsigned long long s_item;
  __shared__ int s_cmd;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int C = a.items_per_batch;
  const int cpw = a.tiles_per_wave * kG32Waves / kW;      // 64-row chunks per wave per item
  if (blockIdx.x == 0) {                                  // doorbell (persist_core.h)
    if (wave == 0) persist_doorbell(a, lane);
    return;                                               // no barrier is ever used by WG 0
  }
  const int T = a.gbdt_trees;
  const G32Model M = g32_model<D>(a.blob, T);
  const float* leaves = g32_leaves<D, kGL>(M, T, lv, tid, 64 * kW);
  epi_init(epi);
  __syncthreads();
  unsigned long long posted_cache = 0;                    // thread 0 only

  G32Wave w;                                              // this wave's share of the item (g32_item_commit)
  // transpose, lift, trees, row epilogue and flag list of one fetched 64-row chunk
  auto score_chunk = [&](const ccfd_persist_desc& d, const PersistItem& it, int chunk, G32Row& cur)
      __attribute__((always_inline)) {
    gx_rows<kG20>(xt[wave], lane, cur);
    unsigned b0[kF];
    const unsigned meta = gx_lift<kG20>(cur, b0);
    float acc[1];
#ifdef CCFD_EXP_READ_ONLY
    // experiment build only: the same items, loads, outputs and protocol with the trees replaced
    // by a use of the bins -- what the persistent read + completion path alone sustains
    acc[0] = (float)(b0[0] + b0[kF - 1]) * 1e-3f;
#else
    g32_trees<D, 1>(b0, b0, leaves, M.feat, M.kbin, T, acc);
#endif
    const int row = chunk * kG32Rows + lane;
    const G32RowOut o = g32_row_epilogue<kR>(epi, w, M, meta, acc[0], row, it.n, a.threshold, a.rules, d.proba, d.route);
    persist_emit_flagged(a, d, it.slot, o.m, o.fr, row, lane);
  };

  for (;;) {
#ifdef CCFD_EXP_ITEM_TRACE
    unsigned long long t_claim = 0, t_claimed = 0, t_seen = 0, t_desc = 0, t_load = 0, t_scored = 0;
    if (tid == 0) {
      t_claim = wall_clock64();
      const unsigned long long it =
          __hip_atomic_fetch_add(&a.dev->work_next, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the claim's value is back (not just issued)
      t_claimed = wall_clock64();
      // persist_wait_item, split: the wait for the posting, then the descriptor read
      const unsigned long long b = it / (unsigned long long)C;
      s_cmd = persist_wait_posted<false>(a, b, posted_cache);
      t_seen = wall_clock64();
      if (!s_cmd) persist_read_desc(a, b, sdesc);
      s_item = it;
      t_desc = wall_clock64();
    }
#else
    if (tid == 0) persist_claim(a, C, posted_cache, sdesc, s_item, s_cmd);
#endif
    __syncthreads();
    if (s_cmd) break;
    const ccfd_persist_desc d = sdesc;                     // registers: no LDS wait in the epilogue
    const PersistItem it = persist_item(a, d, s_item, C, kW * cpw, wave, tid == 0);   // K7: item 0 is claimed first
    const int n = it.n, c0 = it.u0;                       // this wave's chunks: c0 + kW*k
    const unsigned char* xb = it.xb;
    // CCFD_G32_INFLIGHT=1: every chunk of the wave's share of the item in flight at once
    // (static registers: no copy of a pending load, so no vmcnt(0) between chunks)
    auto full_item = [&](auto kC) __attribute__((always_inline)) {
      constexpr int CPW = decltype(kC)::value;
      G32Row r[CPW];
#pragma unroll
      for (int k = 0; k < CPW; ++k) {
        const int chunk = c0 + kW * k;
        if (chunk * kG32Rows < n) gx_fetch<kG20>(xb, n, chunk, lane, r[k]);
      }
#pragma unroll
      for (int k = 0; k < CPW; ++k) {
        const int chunk = c0 + kW * k;
        if (chunk * kG32Rows >= n) break;                 // wave-uniform
        score_chunk(d, it, chunk, r[k]);
      }
    };
    if (a.flags & CCFD_ARG_CHUNK_RING) {                  // default: one chunk ahead
      G32Row pre;
      if (c0 * kG32Rows < n) gx_fetch<kG20>(xb, n, c0, lane, pre);
#pragma unroll 1
      for (int k = 0; k < cpw; ++k) {
        const int chunk = c0 + kW * k;
        if (chunk * kG32Rows >= n) break;                 // wave-uniform
        G32Row cur_row = pre;
        CCFD_ITRACE(if (k == 0) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); if (tid == 0) t_load = wall_clock64(); })
        if (k + 1 < cpw && (chunk + kW) * kG32Rows < n) gx_fetch<kG20>(xb, n, chunk + kW, lane, pre);
        score_chunk(d, it, chunk, cur_row);
      }
    } else if (cpw == 1) {
      full_item(std::integral_constant<int, 1>{});
    } else if (cpw == 2) {
      full_item(std::integral_constant<int, 2>{});
    } else {
      full_item(std::integral_constant<int, 4>{});        // 1024-row items (engine accepts 256/512/1024)
    }
    CCFD_ITRACE(if (tid == 0) t_scored = wall_clock64();)
    g32_item_commit(epi, w, a.counters[d.epoch & 1], lane);
    persist_item_done(a, epi, d, it.slot, C, tid);
#ifdef CCFD_EXP_ITEM_TRACE
    if (tid == 0) {
      const unsigned long long k =
          __hip_atomic_fetch_add(&g_item_trace_n, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      g_item_trace[k % kItemTraceCap] = ItemTrace{s_item, blockIdx.x, t_claim, t_claimed, t_seen, t_desc, t_load, t_scored,
                                                  (unsigned long long)wall_clock64()};
    }
#endif
  }
}

// Pipelined static items (engine persist_items = pipelined / CCFD_PERSIST_PIPE=1; VERDICT r4
// item 6).  The claimed kernel above ends every item with its outputs' release, a ticket and
// then -- only then -- the next claim, descriptor read and first loads: a 512-row G20 item is
// 10 KB, so at ~18 us of loaded PCIe read latency a workgroup has nothing in flight for a
// large share of each item (profiles/r4/g20/README.md).  Here, as in persist_pipe_kernel
// (score_persist.hip) for W64 rows:
//   * worker w (workgroup 1 + w of W) takes items base + w, base + w + W, ... -- no claim
//     atomic, the next item is known;
//   * the next item's rows are issued BEFORE the current item is scored, so its PCIe round
//     trip overlaps the current item's evaluation, output stores, release and ticket (the
//     release's vmcnt drain then waits on loads that are needed next anyway);
//   * leaves in LDS only (kGL = false: BASELINE's 100 x 6 is 25.6 KB); 512-row items (CPW 2).
// Unlike round 4's rejected two-item CLAIM pipeline, nothing is claimed early: the static
// assignment already fixes which workgroup scores which item.
template <int D, bool kR, bool kG20, int CPW>
__global__ __launch_bounds__(256) void persist_gbdt_pipe_kernel(ccfd_persist_args a) {
  extern __shared__ __attribute__((aligned(16))) float lv[];
  __shared__ uint4 xt[kG32Waves][128];
  __shared__ EpilogueLds epi;
  __shared__ ccfd_persist_desc sdesc[2];
  __shared__ int s_pre, s_cmd;                            // rewritten by thread 0 after a barrier only

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int C = a.items_per_batch;
  if (blockIdx.x == 0) {                                  // doorbell (persist_core.h)
    if (wave == 0) persist_doorbell(a, lane);
    return;
  }
  const int T = a.gbdt_trees;
  const G32Model M = g32_model<D>(a.blob, T);
  const float* leaves = g32_leaves<D, false>(M, T, lv, tid, 256);
  epi_init(epi);
  __syncthreads();
  G32Wave w;
  auto issue = [&](const ccfd_persist_desc& d, unsigned long long it, G32Row (&r)[CPW]) __attribute__((always_inline)) {
    const PersistItem i = persist_item(a, d, it, C, kG32Waves * CPW, wave, false);
#pragma unroll
    for (int k = 0; k < CPW; ++k) {
      const int chunk = i.u0 + kG32Waves * k;
      if (chunk * kG32Rows < i.n) gx_fetch<kG20>(i.xb, i.n, chunk, lane, r[k]);
    }
  };
  auto score = [&](const ccfd_persist_desc& ds, unsigned long long it, G32Row (&r)[CPW]) __attribute__((always_inline)) {
    const ccfd_persist_desc d = ds;                       // registers: no LDS reads in the epilogue
    const PersistItem i = persist_item(a, d, it, C, kG32Waves * CPW, wave, false);
#pragma unroll
    for (int k = 0; k < CPW; ++k) {
      const int chunk = i.u0 + kG32Waves * k;
      if (chunk * kG32Rows >= i.n) break;                 // wave-uniform
      gx_rows<kG20>(xt[wave], lane, r[k]);
      unsigned b0[kF];
      const unsigned meta = gx_lift<kG20>(r[k], b0);
      float acc[1];
      g32_trees<D, 1>(b0, b0, leaves, M.feat, M.kbin, T, acc);
      const int row = chunk * kG32Rows + lane;
      const G32RowOut o = g32_row_epilogue<kR>(epi, w, M, meta, acc[0], row, i.n, a.threshold, a.rules, d.proba, d.route);
      persist_emit_flagged(a, d, i.slot, o.m, o.fr, row, lane);
    }
    g32_item_commit(epi, w, a.counters[d.epoch & 1], lane);
    persist_item_done(a, epi, d, i.slot, C, tid);         // barriers, release, ticket
  };
  G32Row ra[CPW], rb[CPW];
  persist_pipe_run(a, C, sdesc, s_pre, s_cmd, ra, rb, issue, score);
}

template <int D, bool kG20>
static int launch_persist_g32_f(const ccfd_persist_args& a0, int grid, hipStream_t s) {
  ccfd_persist_args a = a0;
  // one-chunk prefetch ring by default: at BASELINE config 4 (65536-row batches) it measured
  // 1.67e9 tx/s at p50 107 us (depth 3) vs 1.64e9 with the whole item in flight (VALU-heavy
  // trees overlap the next chunk's load better); CCFD_G32_INFLIGHT=1 selects the latter.
  // Read per launch: sweepable in-process (profiles/r2/persist_full_item/g32_inflight_ab.jsonl)
  if (g32_env("CCFD_G32_INFLIGHT", 0, 0, 1) == 0) a.flags |= CCFD_ARG_CHUNK_RING;
  const bool gl = ((long)a.gbdt_trees << D) > kG32LeafLds || g32_env("CCFD_G32_GLOBAL_LEAVES", 0, 0, 1);
  const size_t lds = gl ? 0 : (size_t)a.gbdt_trees * (1 << D) * sizeof(float);
  const bool pipe = (a.flags & CCFD_ARG_PIPE_ITEMS) != 0;   // pipelined static 512-row items
  if (pipe && (gl || a.tiles_per_wave != 2 || grid < 2)) return -2;
  dispatch_bool(a.rules != nullptr, [&](auto kr) {
    constexpr bool kR = decltype(kr)::value;
    if (pipe) {
      hipLaunchKernelGGL((persist_gbdt_pipe_kernel<D, kR, kG20, 2>), dim3(grid), dim3(256), lds, s, a);
      return;
    }
#ifdef CCFD_EXP_G20_WAVES8
    if (!gl && a.tiles_per_wave % 2 == 0) {
      hipLaunchKernelGGL((persist_gbdt_g32_kernel<D, kR, false, kG20, 8>), dim3(grid), dim3(512), lds, s, a);
      return;
    }
#endif
    dispatch_bool(gl, [&](auto kgl) {                     // lds == 0 with global leaves
      hipLaunchKernelGGL((persist_gbdt_g32_kernel<D, kR, decltype(kgl)::value, kG20>), dim3(grid), dim3(256), lds, s, a);
    });
  });
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

#ifdef CCFD_EXP_ITEM_TRACE
// host: the item ring -> <path> as {u64 n, ItemTrace[kItemTraceCap]} (record k at k % cap), then the
// doorbell ring (persist_core.h)
int item_trace_dump(const char* path) {
  unsigned long long n = 0;
  std::vector<ItemTrace> v(kItemTraceCap);
  if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_item_trace_n), sizeof(n)) != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(v.data(), HIP_SYMBOL(g_item_trace), sizeof(ItemTrace) * v.size()) != hipSuccess) return -1;
  FILE* f = std::fopen(path, "wb");
  if (!f) return -1;
  std::fwrite(&n, sizeof(n), 1, f);
  std::fwrite(v.data(), sizeof(ItemTrace), v.size(), f);
  // then the doorbell ring: {u64 n, DoorbellTrace[kDoorbellTraceCap]}
  std::vector<DoorbellTrace> db(kDoorbellTraceCap);
  unsigned long long ndb = 0;
  if (hipMemcpyFromSymbol(&ndb, HIP_SYMBOL(g_db_trace_n), sizeof(ndb)) == hipSuccess &&
      hipMemcpyFromSymbol(db.data(), HIP_SYMBOL(g_db_trace), sizeof(DoorbellTrace) * db.size()) == hipSuccess) {
    std::fwrite(&ndb, sizeof(ndb), 1, f);
    std::fwrite(db.data(), sizeof(DoorbellTrace), db.size(), f);
  }
  std::fclose(f);
  return 0;
}
#endif

int launch_persist_gbdt_g32(const ccfd_persist_args& a, int grid, hipStream_t s) {
  if (a.gbdt_trees <= 0 || a.gbdt_depth < 1 || a.gbdt_depth > 8) return -2;
  return dispatch_depth(a.gbdt_depth, [&](auto d) {
    return dispatch_bool((a.flags & CCFD_ARG_WIRE_G20) != 0, [&](auto g20) {
      return launch_persist_g32_f<decltype(d)::value, decltype(g20)::value>(a, grid, s);
    });
  });
}

}  // namespace ccfd

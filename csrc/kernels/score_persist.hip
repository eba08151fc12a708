// Persistent streaming scorer (engine exec_mode = 1), MLP and LR; protocol helpers in
// persist_core.h (the GBDT G32 persistent kernel shares them, score_gbdt_g32_persist.hip).
//
// One launch lives as long as the engine.  Every resident workgroup loops:
//   claim work item i (one agent-scope atomic)      -> micro-batch b = i / C, chunk c = i % C
//   wait until b is posted                          (thread 0 polls the DEVICE mirror kept by
//                                                   the doorbell workgroup 0, which alone
//                                                   polls host memory with relaxed system-
//                                                   scope loads; s_sleep back-off)
//   read descriptor b % R from the device mirror    -> LDS
//   4 waves x T tiles x 16 rows (item = 64T rows, CCFD_PERSIST_ITEM_ROWS; engine defaults
//   T = 8 for the MLP on W64 rows, 4 otherwise): W64 items of 4 / 8 tiles issue every tile
//   at once and score them in pairs, other sizes prefetch the next tile while the current
//   one computes (f32 rows via a wave-private LDS tile); the same fused math as the
//   per-batch kernels (mlp_core.h), outputs written straight to host-mapped memory,
//   fraud rows appended to the descriptor's compacted flag list (row epilogue: tile_core.h)
//   counters + amount histogram -> counters[desc.epoch] (one atomic set per item)
//   release (system scope) + ticket on remaining[b % R]; the last ticket publishes
//   ctl->done[b % R] = {b + 1, #flagged, t_start, t_end}
// A workgroup only waits for the HOST (never for another workgroup), so residency of the
// whole grid is not required and nothing can deadlock; it exits when the host sets `stop`
// while it waits for an unposted batch.  The host never posts batch b into ring slot
// b % R before observing done for b - R, which is what makes the slot-local state
// (remaining/nflag reset by the last ticket) safe to reuse.
#include <type_traits>

#include "lr_core.h"
#include "mlp_core.h"
#include "persist_core.h"
#include "rules.h"
#include "tile_core.h"

namespace ccfd {

int launch_persist_gbdt_g32(const ccfd_persist_args& a, int grid, hipStream_t s);   // score_gbdt_g32_persist.hip

namespace {

template <int kModel, bool kR>
__global__ __launch_bounds__(256) void persist_kernel(ccfd_persist_args a) {
  __shared__ __attribute__((aligned(16))) char sblob[kMlpBlobWire];
  __shared__ __attribute__((aligned(16))) float sx[4][kTileRows * kF + 4];
  __shared__ EpilogueLds epi;
  __shared__ ccfd_persist_desc sdesc;
  __shared__ unsigned long long s_item;
  __shared__ int s_cmd;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int C = a.items_per_batch;

  if (kModel == CCFD_MODEL_MLP)
    mlp_stage(a.blob, sblob, tid, 256, (a.flags & CCFD_ARG_WIRE_W64) ? kMlpBlobWire : kMlpBlob);
  else for (int i = tid; i < kLrBlob / 16; i += 256) reinterpret_cast<int4*>(sblob)[i] = reinterpret_cast<const int4*>(a.blob)[i];
  epi_init(epi);
  __syncthreads();

  MlpLane L{};
  MlpWireLane LW{};
  LrLane LL{};
  if (kModel == CCFD_MODEL_MLP) {
    L = mlp_lane(sblob, g);
    LW = mlp_wire_lane(sblob);
  } else {
    LL = lr_lane(sblob, g);
  }
  float* tile_lds = sx[wave];
  TileWave w;                              // this wave's share of the item (tile_item_commit)
  unsigned long long posted_cache = 0;     // thread 0 only

  // Workgroup 0 is the DOORBELL (persist_core.h): its first wave alone polls host memory.
  if (blockIdx.x == 0) {
    if (wave == 0) persist_doorbell(a, lane);
    return;                                              // no barrier is ever used by WG 0
  }

  for (;;) {
    if (tid == 0) persist_claim(a, C, posted_cache, sdesc, s_item, s_cmd);
    __syncthreads();
    if (s_cmd) break;

    // the item's descriptor in registers: the epilogue reads its pointers with no LDS wait
    const ccfd_persist_desc dsc = sdesc;
    const int kTilesPerWave = a.tiles_per_wave;
    const PersistItem it = persist_item(a, dsc, s_item, C, 4 * kTilesPerWave, wave, tid == 0);   // K7: item 0 is claimed first
    const int slot = it.slot, n = it.n, tile0 = it.u0;         // wave w: tiles tile0 + 4k
    const float* x = dsc.x;
    auto avail = [&](int t) { return min(kTileRows, n - t * kTileRows) * kF * 4; };
    const bool wire = (a.flags & CCFD_ARG_WIRE_W64) != 0;       // uniform per launch
    const unsigned char* xw = it.xb;
    // per-tile epilogue (tile_core.h) and the compacted fraud list; xr = the tile's raw
    // features (routing rules only)
    auto finish = [&](float p, float amount, int tile, float (&xr)[8]) __attribute__((always_inline)) {
      const int row = tile * kTileRows + c;
      bool rf;
      if constexpr (kR) {                               // configurable routing rules (rules.h)
        const float pr = __shfl(p, c);
        rf = row < n && (wire ? rule_route(a.rules, pr, [&](int j) { return lane_feature<true>(xr, j, c); })
                              : rule_route(a.rules, pr, [&](int j) { return lane_feature<false>(xr, j, c); }));
      } else {
        rf = p >= a.threshold;
      }
      const TileRowOut o = tile_row_epilogue(epi, w, p, rf, amount, row, n, g, dsc.proba, dsc.route);
      persist_emit_flagged(a, dsc, slot, o.m, o.fr && g == 0, row, lane);
    };
    // W64 items of 2, 4 or 8 tiles per wave (128 / 256 / 512 rows): every tile
    // of the item in flight at once -- the item costs one PCIe round trip instead of one per
    // tile, so fewer rows in flight keep the link busy (lower p50 at the same rate) -- and
    // scored in pairs (mlp_tile_w64_x2: one LDS weight read feeds two MFMAs)
    auto full_item = [&](auto kT) __attribute__((always_inline)) {
      constexpr int T = decltype(kT)::value;
      WireRegs r[T];
#pragma unroll
      for (int k = 0; k < T; ++k) wire_issue(xw, n, tile0 + 4 * k, c, g, r[k]);
#pragma unroll
      for (int k = 0; k < T; k += 2) {
        const int ta = tile0 + 4 * k;
        if (ta * kTileRows >= n) break;                    // wave-uniform
        float pa, pb;
        float xa[8], xb[8];
        if (kModel == CCFD_MODEL_MLP) {
          mlp_tile_w64_x2(sblob, LW, r[k], r[k + 1], g, lane, pa, pb);
          if constexpr (kR) { wire_features(r[k], g, xa); wire_features(r[k + 1], g, xb); }
        } else {
          wire_features(r[k], g, xa);
          wire_features(r[k + 1], g, xb);
          float la[8], lb[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) { la[j] = xa[j]; lb[j] = xb[j]; }
          pa = lr_proba(LL, la, g);
          pb = lr_proba(LL, lb, g);
        }
        finish(pa, __uint_as_float(r[k].v.w), ta, xa);
        finish(pb, __uint_as_float(r[k + 1].v.w), ta + 4, xb);   // rows >= n: no-op epilogue
      }
    };
    if (wire && kTilesPerWave == 2) {
      full_item(std::integral_constant<int, 2>{});
    } else if (wire && kTilesPerWave == 4) {
      full_item(std::integral_constant<int, 4>{});
    } else if (wire && kTilesPerWave == 8) {
      full_item(std::integral_constant<int, 8>{});
    } else {
      TileRegs pre;
      WireRegs wpre;
      if (tile0 * kTileRows < n) {
        if (wire) wire_issue(xw, n, tile0, c, g, wpre);
        else tile_issue(x + (size_t)tile0 * kTileRows * kF, avail(tile0), lane, pre);
      }
#pragma unroll 1
      for (int k = 0; k < kTilesPerWave; ++k) {
        const int tile = tile0 + 4 * k;
        const int row0 = tile * kTileRows;
        if (row0 >= n) break;                                // wave-uniform
        const int nxt = tile + 4;
        float xv[8];
        WireRegs cur_w;
        if (wire) {
          cur_w = wpre;
          if (k + 1 < kTilesPerWave && nxt * kTileRows < n) wire_issue(xw, n, nxt, c, g, wpre);
          if (kModel != CCFD_MODEL_MLP || kR) wire_features(cur_w, g, xv);
        } else {
          tile_store(tile_lds, lane, pre);
          if (k + 1 < kTilesPerWave && nxt * kTileRows < n) tile_issue(x + (size_t)nxt * kTileRows * kF, avail(nxt), lane, pre);
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
          tile_features(tile_lds, c, g, xv);
        }
        float xr[8];                                         // raw features for the rules
        if constexpr (kR) {
#pragma unroll
          for (int j = 0; j < 8; ++j) xr[j] = xv[j];
        }
        float p, amount;
        if (kModel == CCFD_MODEL_MLP) {
          if (wire) {        // W64 blob: raw bf16 operands, folded normalisation (mlp_core.h)
            amount = __uint_as_float(cur_w.v.w);
            p = mlp_tile_w64(sblob, LW, cur_w, g, lane);
          } else {
            p = mlp_tile(sblob, L, xv, g, lane, amount);
            if (kR && g == 3) xr[5] = amount;              // the model replaced Amount by its log1p
          }
        } else {
          amount = xv[5];
          p = lr_proba(LL, xv, g);
        }
        finish(p, amount, tile, xr);
      }
    }
    tile_item_commit(epi, w, lane);
    persist_item_done(a, epi, dsc, slot, C, tid);
  }
}

// Pipelined static work items (CCFD_ARG_PIPE_ITEMS; MLP on W64 rows; the pipeline itself is
// persist_pipe_run, persist_core.h).  A CU reading host
// memory sustains only ~2 GB/s (a few KB of requests outstanding over a ~2 us PCIe round
// trip), so a micro-batch finishes soonest when its 256 KB is spread over many CUs: small
// items (64 / 128 rows, one per workgroup).  The claim-score-release chain of one item is
// ~9 us of latency, though (atomic claim, descriptor read, PCIe round trip, output release,
// ticket), which with one item per workgroup at a time capped small items far below the link
// (profiles/r3/latency/latency_sweep_workgroup_items.jsonl).  Here:
//   * items are assigned statically -- worker w (workgroup 1 + w of W) takes items
//     base + w, base + w + W, ... -- so there is no claim atomic and a worker knows its next
//     item without asking;
//   * while item i is scored, the descriptor of item i + W is read and its rows are already
//     in flight (when its micro-batch is posted), so one item's release / ticket overlaps the
//     next item's PCIe round trip;
//   * a worker waiting for a batch several batches ahead of the posted count sleeps longer,
//     so idle workers do not hammer the device `posted` word.
// T = tiles per wave per item (1: 64-row items, 2: 128-row items).
template <bool kR, int T>
__global__ __launch_bounds__(256) void persist_pipe_kernel(ccfd_persist_args a) {
  static_assert(T == 1 || T == 2, "64- or 128-row items");
  __shared__ __attribute__((aligned(16))) char sblob[kMlpBlobWire];
  __shared__ EpilogueLds epi;
  __shared__ ccfd_persist_desc sdesc[2];
  __shared__ int s_pre, s_cmd;                           // rewritten by thread 0 after a barrier only

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int C = a.items_per_batch;
  mlp_stage(a.blob, sblob, tid, 256, kMlpBlobWire);
  epi_init(epi);
  __syncthreads();
  if (blockIdx.x == 0) {                                 // the DOORBELL (persist_core.h)
    if (wave == 0) persist_doorbell(a, lane);
    return;
  }
  const MlpWireLane LW = mlp_wire_lane(sblob);
  TileWave w;

  auto issue = [&](const ccfd_persist_desc& d, unsigned long long it, WireRegs (&r)[T]) __attribute__((always_inline)) {
    const PersistItem i = persist_item(a, d, it, C, 4 * T, wave, false);   // wave w: tiles u0 + 4k
#pragma unroll
    for (int k = 0; k < T; ++k) wire_issue(i.xb, i.n, i.u0 + 4 * k, c, g, r[k]);
  };
  // score item `it` (rows in r), counters into LDS, outputs to the host, then release + ticket
  auto score = [&](const ccfd_persist_desc& d, unsigned long long it, WireRegs (&r)[T]) __attribute__((always_inline)) {
    const PersistItem i = persist_item(a, d, it, C, 4 * T, wave, false);
    const int n = i.n, tile0 = i.u0;
    auto finish = [&](float p, const WireRegs& rr, int tile) __attribute__((always_inline)) {
      const int row = tile * kTileRows + c;
      bool rf;
      if constexpr (kR) {
        float xr[8];
        wire_features(rr, g, xr);
        rf = row < n && rule_route(a.rules, __shfl(p, c), [&](int j) { return lane_feature<true>(xr, j, c); });
      } else {
        rf = p >= a.threshold;
      }
      const TileRowOut o = tile_row_epilogue(epi, w, p, rf, __uint_as_float(rr.v.w), row, n, g, d.proba, d.route);
      persist_emit_flagged(a, d, i.slot, o.m, o.fr && g == 0, row, lane);
    };
    if (tile0 * kTileRows < n) {
      if constexpr (T == 2) {
        float pa, pb;
        mlp_tile_w64_x2(sblob, LW, r[0], r[1], g, lane, pa, pb);
        finish(pa, r[0], tile0);
        finish(pb, r[1], tile0 + 4);                     // rows >= n: no-op epilogue
      } else {
        finish(mlp_tile_w64(sblob, LW, r[0], g, lane), r[0], tile0);
      }
    }
    tile_item_commit(epi, w, lane);
    persist_item_done(a, epi, d, i.slot, C, tid);
  };
  WireRegs ra[T], rb[T];
  persist_pipe_run(a, C, sdesc, s_pre, s_cmd, ra, rb, issue, score);
}

}  // namespace

}  // namespace ccfd

extern "C" int ccfd_persist_launch(const ccfd_persist_args* a, int grid, void* stream) {
  using namespace ccfd;
  if (!a || !a->ctl || !a->desc || !a->dev || !a->blob) return -1;
  if (a->ring <= 0 || a->ring > CCFD_PERSIST_MAX_RING || a->items_per_batch <= 0 || a->tiles_per_wave <= 0) return -2;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool pipe = a->model == CCFD_MODEL_MLP && (a->flags & CCFD_ARG_PIPE_ITEMS);
  if (pipe && (!(a->flags & CCFD_ARG_WIRE_W64) || grid < 2 || a->tiles_per_wave < 1 || a->tiles_per_wave > 2)) return -2;
  if (a->model == CCFD_MODEL_GBDT && (a->flags & CCFD_ARG_WIRE_G32)) return launch_persist_gbdt_g32(*a, grid, s);
  if (a->model != CCFD_MODEL_MLP && a->model != CCFD_MODEL_LR) return -3;
  // routing rules: separate instantiations, so threshold-only kernels keep their registers
  dispatch_bool(a->rules != nullptr, [&](auto kr) {
    constexpr bool kR = decltype(kr)::value;
    const dim3 g(grid), b(256);
    if (pipe && a->tiles_per_wave == 1) hipLaunchKernelGGL((persist_pipe_kernel<kR, 1>), g, b, 0, s, *a);
    else if (pipe) hipLaunchKernelGGL((persist_pipe_kernel<kR, 2>), g, b, 0, s, *a);
    else if (a->model == CCFD_MODEL_MLP) hipLaunchKernelGGL((persist_kernel<CCFD_MODEL_MLP, kR>), g, b, 0, s, *a);
    else hipLaunchKernelGGL((persist_kernel<CCFD_MODEL_LR, kR>), g, b, 0, s, *a);
  });
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

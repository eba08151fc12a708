// Shadow scoring: a challenger MLP scored beside the champion in the same pass over the rows.
//
// The streaming path is bound by the bytes a row costs on the link, not by model math, so the
// way to tell what a hot swap would do to live traffic is to score the candidate on the very
// rows the champion is scoring: both W64 weight blobs are staged in LDS once per workgroup and
// every 16-row tile (or tile pair) held in registers goes through the MFMA chain twice, once
// per LDS base.  The rows are read once; a second launch would read them twice.
//
// Both kernels run the champion's device functions (mlp_core.h) unchanged for the challenger
// -- only the LDS base and the per-blob lane constants differ -- so rows scored with blob B as
// the shadow carry the same bits as rows scored with B as the champion.
//
//   * score_shadow_kernel: one launch per micro-batch (plain launches, score_sync, the engine's
//     exec_mode launch).  Champion epilogue as in wire_body.h (tile_row_epilogue_lanes of
//     tile_core.h: outputs, route, counters, amount histogram; staged flag list, completion
//     record).
//   * persist_shadow_kernel: the claimed-item path of score_persist.hip for W64 items of 2, 4
//     or 8 tiles per wave, protocol helpers of persist_core.h unchanged: a workgroup waits only
//     for the host and leaves on `stop`; workgroup 0 is the doorbell.
//
// The challenger adds five counters (CCFD_CNT_SHADOW_*), accumulated per wave, then per
// workgroup in LDS, then one set of atomics per workgroup (launch) or item (persistent); the
// launch kernel also stores its proba_1 per row when asked to.  MLP on W64 rows, threshold
// route only; the two entry points at the end of this file also hand an oblivious-GBDT pair on
// G32 / G20 rows to its own kernels (score_gbdt_shadow.hip).  Everything else is refused on
// the host.
#include <string>
#include <type_traits>

#include "mlp_core.h"
#include "persist_core.h"
#include "shadow_core.h"
#include "tile_core.h"

namespace ccfd {

void set_error(const std::string& e);   // dispatch.hip
int launch_gbdt_shadow(const ccfd_shadow_args& sa, hipStream_t s);                         // score_gbdt_shadow.hip
int launch_persist_gbdt_shadow(const ccfd_persist_shadow_args& sa, int grid, hipStream_t s);

namespace {

constexpr int kShadowWaves = 4;          // waves per workgroup of the launch kernel
// One tile pair per wave until the grid covers the chip: a CU reading host memory sustains only
// a few GB/s, so a 4096-row micro-batch (256 tiles) is spread over 32 workgroups; past one
// workgroup per CU the grid-stride loop takes over (each workgroup stages 56 KB of weights).
constexpr int kShadowTilesPerWave = 2;
constexpr int kShadowGridCap = 256;

// ---------------------------------------------------------------------------------------
// Launch kernel.  Wave w of workgroup b streams tiles b * kWaves + w + k * tstride with a
// two-tile prefetch ring: the steady-state loop scores the pair in the ring against both
// blobs (mlp_tile_w64_x2: one LDS weight read feeds two MFMAs) and refills both slots before
// the epilogue; at most one tile is left for the tail (mlp_tile_w64).  Loads are branch-free
// (rows clamped into the batch; clamped rows are never scored), as in wire_body.h.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * kShadowWaves) void score_shadow_kernel(ccfd_shadow_args sa) {
  constexpr int kWaves = kShadowWaves;
  __shared__ __attribute__((aligned(16))) char lds[2][kMlpBlobWire];
  __shared__ EpilogueLds epi;
  __shared__ ShadowLds sh;
  __shared__ unsigned flbuf[kWaves][128];
  const ccfd_score_args& a = sa.base;
  const int blk = blockIdx.x, nblk = gridDim.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  stamp_start(a, blk);
  const int n = a.n;
  const int ntiles = (n + kTileRows - 1) / kTileRows;
  const int tstride = nblk * kWaves;
  int tile = blk * kWaves + wave;
  const unsigned char* xw = reinterpret_cast<const unsigned char*>(a.x) + 16 * g;
  auto issue = [&](int t, WireRegs& r) __attribute__((always_inline)) {
    const int row = min(t * kTileRows + c, n - 1);
    r.v = ld_g16(xw + (size_t)row * CCFD_WIRE_ROW_BYTES);
  };
  // the first pair's (possibly PCIe) fetch overlaps the staging of the two blobs
  WireRegs r0, r1;
  issue(tile, r0);
  issue(tile + tstride, r1);
  mlp_stage(a.blob, lds[0], tid, 64 * kWaves, kMlpBlobWire);
  mlp_stage(sa.shadow_blob, lds[1], tid, 64 * kWaves, kMlpBlobWire);
  epi_init(epi);
  shadow_init(sh);
  __syncthreads();
  const MlpWireLane LA = mlp_wire_lane(lds[0]);
  const MlpWireLane LB = mlp_wire_lane(lds[1]);

  const float thr = a.threshold;
  FlagStage fls{flbuf[wave], 0u};
  TileWave w;
  ShadowAcc sw;
  HistLanes hl;
  hist_lanes_init(hl, g);
  // p: champion, q: challenger proba_1 of row c of tile t (identical in the 4 lane groups):
  // the champion's epilogue, then the challenger's output and counts
  auto finish = [&](float p, float q, float amount, int t) __attribute__((always_inline)) {
    const int row = t * kTileRows + c;
    const TileRowOut o = tile_row_epilogue_lanes(epi, w, hl, p, p >= thr, amount, t, n, g, c, a.proba, a.route);
    const bool sf = o.valid && (q >= thr);
    if (o.valid && g == 0) {
      if (sa.shadow_proba) st_g(sa.shadow_proba + row, q);
      shadow_row(sw, p, q);
    }
    sw.fraud += __popcll(__ballot(sf && g == 3));
    sw.both += __popcll(__ballot(sf && o.fr && g == 3));
    if (o.m) flag_push(a, fls, o.m, o.fr && g == 3, row, lane);
  };
  // steady state: both tiles of the pair exist
  const int full_end = ntiles - tstride;
  while (tile < full_end) {
    const float am0 = __uint_as_float(r0.v.w), am1 = __uint_as_float(r1.v.w);
    float p0, p1, q0, q1;
    mlp_tile_w64_x2(lds[0], LA, r0, r1, g, lane, p0, p1);
    mlp_tile_w64_x2(lds[1], LB, r0, r1, g, lane, q0, q1);
    issue(tile + 2 * tstride, r0);
    issue(tile + 3 * tstride, r1);
    finish(p0, q0, am0, tile);
    finish(p1, q1, am1, tile + tstride);
    tile += 2 * tstride;
  }
  // tail: at most one tile left, already in r0
  if (tile < ntiles) {
    const float p = mlp_tile_w64(lds[0], LA, r0, g, lane);
    const float q = mlp_tile_w64(lds[1], LB, r0, g, lane);
    finish(p, q, __uint_as_float(r0.v.w), tile);
  }
  if (a.flag_idx != nullptr) flag_flush(a, fls, lane);
  hist_lanes_commit(epi, hl, g, c);
  const unsigned rows = w.rows;
  tile_wave_commit(epi, w, lane);
  shadow_wave_commit(sh, sw, rows, lane);
  epi_flush_ballot(epi, a.counters);                    // barrier first, then the champion's atomics
  if (tid == 2 * kNB + 1) shadow_flush(sh, a.counters);
  signal_done(a, (unsigned)nblk);
}

// ---------------------------------------------------------------------------------------
// Persistent kernel: persist_kernel's full_item path (score_persist.hip) with both blobs
// staged once per resident workgroup.  Every tile of the claimed item is in flight at once
// and scored in pairs, first against the champion, then against the challenger.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void persist_shadow_kernel(ccfd_persist_shadow_args sa) {
  __shared__ __attribute__((aligned(16))) char sblob[2][kMlpBlobWire];
  __shared__ EpilogueLds epi;
  __shared__ ShadowLds sh;
  __shared__ ccfd_persist_desc sdesc;
  __shared__ unsigned long long s_item;
  __shared__ int s_cmd;
  const ccfd_persist_args& a = sa.base;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int C = a.items_per_batch;

  mlp_stage(a.blob, sblob[0], tid, 256, kMlpBlobWire);
  mlp_stage(sa.shadow_blob, sblob[1], tid, 256, kMlpBlobWire);
  epi_init(epi);
  shadow_init(sh);
  __syncthreads();
  const MlpWireLane LA = mlp_wire_lane(sblob[0]);
  const MlpWireLane LB = mlp_wire_lane(sblob[1]);
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

    const ccfd_persist_desc dsc = sdesc;
    const int kTilesPerWave = a.tiles_per_wave;
    const PersistItem it = persist_item(a, dsc, s_item, C, 4 * kTilesPerWave, wave, tid == 0);   // K7: item 0 is claimed first
    const int slot = it.slot, n = it.n, tile0 = it.u0;         // wave w: tiles tile0 + 4k
    const unsigned char* xw = it.xb;
    TileWave w;
    ShadowAcc sw;
    // per-tile epilogue: the champion's as in persist_kernel (tile_core.h), then the challenger's counters
    auto finish = [&](float p, float q, float amount, int tile) __attribute__((always_inline)) {
      const int row = tile * kTileRows + c;
      const TileRowOut o = tile_row_epilogue(epi, w, p, p >= a.threshold, amount, row, n, g, dsc.proba, dsc.route);
      const bool sf = o.valid && (q >= a.threshold);
      if (o.valid && g == 0) shadow_row(sw, p, q);
      sw.fraud += __popcll(__ballot(sf && g == 0));
      sw.both += __popcll(__ballot(sf && o.fr && g == 0));
      persist_emit_flagged(a, dsc, slot, o.m, o.fr && g == 0, row, lane);
    };
    auto full_item = [&](auto kT) __attribute__((always_inline)) {
      constexpr int T = decltype(kT)::value;
      WireRegs r[T];
#pragma unroll
      for (int k = 0; k < T; ++k) wire_issue(xw, n, tile0 + 4 * k, c, g, r[k]);
#pragma unroll
      for (int k = 0; k < T; k += 2) {
        const int ta = tile0 + 4 * k;
        if (ta * kTileRows >= n) break;                    // wave-uniform
        float pa, pb, qa, qb;
        mlp_tile_w64_x2(sblob[0], LA, r[k], r[k + 1], g, lane, pa, pb);
        mlp_tile_w64_x2(sblob[1], LB, r[k], r[k + 1], g, lane, qa, qb);
        finish(pa, qa, __uint_as_float(r[k].v.w), ta);
        finish(pb, qb, __uint_as_float(r[k + 1].v.w), ta + 4);   // rows >= n: no-op epilogue
      }
    };
    // the host launches this kernel with 2, 4 or 8 tiles per wave only
    if (kTilesPerWave == 2) {
      full_item(std::integral_constant<int, 2>{});
    } else if (kTilesPerWave == 4) {
      full_item(std::integral_constant<int, 4>{});
    } else {
      full_item(std::integral_constant<int, 8>{});
    }
    const unsigned nv_w = w.rows;
    tile_item_commit(epi, w, lane);
    shadow_wave_commit(sh, sw, nv_w, lane);
    // the item's challenger counters, then LDS reset for the next item: persist_item_done's
    // barriers and its vmcnt(0) drain order both before the item's ticket and the next claim
    __syncthreads();
    if (tid == 96) {
      shadow_flush(sh, a.counters[dsc.epoch & 1]);
      sh.rows = 0; sh.fraud = 0; sh.both = 0; sh.psum_e6 = 0; sh.absdiff_e6 = 0;
    }
    persist_item_done(a, epi, dsc, slot, C, tid);
  }
}

}  // namespace

}  // namespace ccfd

extern "C" int ccfd_score_launch_shadow(const ccfd_shadow_args* sa, void* stream) {
  using namespace ccfd;
  if (sa == nullptr || sa->base.blob == nullptr || sa->base.x == nullptr || sa->shadow_blob == nullptr) {
    set_error("shadow launch: null argument");
    return -1;
  }
  const ccfd_score_args& a = sa->base;
  if (a.n < 0) { set_error("n < 0"); return -1; }
  if (a.rules != nullptr) { set_error("shadow launch: threshold route only (routing rules refused)"); return -3; }
  if (a.model == CCFD_MODEL_GBDT) {                  // oblivious GBDT pair on binned rows
    if (!(a.flags & CCFD_ARG_WIRE_G32) || (a.flags & CCFD_ARG_WIRE_W64)) {
      set_error("shadow launch: a GBDT pair needs G32 / G20 rows (GBDT on f32 rows refused)");
      return -3;
    }
    if (reinterpret_cast<uintptr_t>(a.x) & ((a.flags & CCFD_ARG_WIRE_G20) ? 3 : 15)) {
      set_error("G32 rows must be 16-byte aligned, G20 rows 4-byte aligned");
      return -3;
    }
    const int rc = launch_gbdt_shadow(*sa, reinterpret_cast<hipStream_t>(stream));
    if (rc == -2) set_error("shadow launch: GBDT shape refused (trees >= 1, depth 1..8)");
    else if (rc) set_error("shadow launch: GBDT kernel launch failed");
    return rc;
  }
  if (a.model != CCFD_MODEL_MLP) {
    set_error(a.model == CCFD_MODEL_LR ? "shadow launch: LR models have no shadow kernel (MLP on W64 rows, GBDT on G32 / G20 rows)"
              : a.model == CCFD_MODEL_FOREST
                  ? "shadow launch: forest models have no shadow kernel (MLP on W64 rows, GBDT on G32 / G20 rows)"
                  : "shadow launch: model kind refused (MLP on W64 rows, GBDT on G32 / G20 rows)");
    return -3;
  }
  if (!(a.flags & CCFD_ARG_WIRE_W64) || (a.flags & (CCFD_ARG_WIRE_G32 | CCFD_ARG_WIRE_G20))) {
    set_error("shadow launch: an MLP pair needs W64 rows (f32 / G32 / G20 rows refused)");
    return -3;
  }
  if (reinterpret_cast<uintptr_t>(a.x) & 15) { set_error("W64 rows must be 16-byte aligned"); return -3; }
  if (a.n == 0) return 0;
  const int ntiles = (a.n + kTileRows - 1) / kTileRows;
  const int per_wg = kShadowWaves * kShadowTilesPerWave;
  int grid = (ntiles + per_wg - 1) / per_wg;
  grid = grid > kShadowGridCap ? kShadowGridCap : grid;
  hipLaunchKernelGGL(score_shadow_kernel, dim3(grid), dim3(64 * kShadowWaves), 0, reinterpret_cast<hipStream_t>(stream),
                     *sa);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error(std::string("kernel launch failed: ") + hipGetErrorString(e)); return -5; }
  return 0;
}

extern "C" int ccfd_persist_launch_shadow(const ccfd_persist_shadow_args* sa, int grid, void* stream) {
  using namespace ccfd;
  if (!sa || !sa->base.ctl || !sa->base.desc || !sa->base.dev || !sa->base.blob || !sa->shadow_blob) return -1;
  const ccfd_persist_args& a = sa->base;
  if (a.ring <= 0 || a.ring > CCFD_PERSIST_MAX_RING || a.items_per_batch <= 0 || grid < 2) return -2;
  if ((a.flags & CCFD_ARG_PIPE_ITEMS) || a.rules) return -3;
  if (a.model == CCFD_MODEL_GBDT) {                  // oblivious GBDT pair on binned rows, items of 1 / 2 / 4 chunks a wave
    if (!(a.flags & CCFD_ARG_WIRE_G32) || (a.flags & CCFD_ARG_WIRE_W64)) return -3;
    if (a.tiles_per_wave != 1 && a.tiles_per_wave != 2 && a.tiles_per_wave != 4) return -2;
    return launch_persist_gbdt_shadow(*sa, grid, reinterpret_cast<hipStream_t>(stream));
  }
  if (a.model != CCFD_MODEL_MLP || !(a.flags & CCFD_ARG_WIRE_W64)) return -3;
  if (a.tiles_per_wave != 2 && a.tiles_per_wave != 4 && a.tiles_per_wave != 8) return -2;
  hipLaunchKernelGGL(persist_shadow_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *sa);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

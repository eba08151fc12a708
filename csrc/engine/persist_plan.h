// How a persistent kernel's work is cut: rows per work item, tiles per wave, claimed or
// pipelined items, items per micro-batch, resident workgroups.  One pure function of the
// engine's configuration and the two environment switches, so every rule (and the measurement
// behind it) is in one place and csrc/tests/persist_plan_check.cpp can check the whole table
// without a GPU (tests/test_native_cpu.py).  Header-only and HIP-free.
#pragma once
#include <cstdlib>

#include "../include/ccfd_abi.h"

namespace ccfd {

struct PersistPlan {
  int item_rows = 0;
  int tiles_per_wave = 1;
  bool pipe = false;           // pipelined static items (CCFD_ARG_PIPE_ITEMS), else claimed
  int items_per_batch = 0;     // ceil(max_batch / item_rows)
  int grid = 0;                // resident workgroups (+ the doorbell)
  bool big_trees = false;      // G32 / G20 GBDT of more than 1200 tree levels a row
};

// `wire`: 0 f32, 1 W64, 2 G32, 3 G20 rows (ccfd_engine_config.wire).  `env_item_rows` /
// `env_pipe`: the values of CCFD_PERSIST_ITEM_ROWS / CCFD_PERSIST_PIPE, nullptr when unset.
inline PersistPlan persist_plan(int model, int wire, int gbdt_trees, int gbdt_depth, int max_batch,
                                int persist_items, int persist_grid, const char* env_item_rows,
                                const char* env_pipe) {
  PersistPlan pl;
  const bool g32 = model == CCFD_MODEL_GBDT && wire >= 2;     // G32 or G20 rows
  const bool w64 = wire == 1;
  const int env_rows = env_item_rows ? std::atoi(env_item_rows) : 0;
  // work-item size: 64 rows (one 16-row tile per wave) by default; CCFD_PERSIST_ITEM_ROWS
  // = 128/256 gives each wave 2/4 tiles with a one-tile prefetch (fewer claims per batch)
  // GBDT on G32 rows: items of 4 waves x 64-row chunks (256 / 512 / 1024 rows, default 512)
  // W64 rows on 64 workgroups, every tile of an item in flight at once (score_persist.hip):
  // MLP 512-row items -- 8.63e8 tx/s at p50 53 us and depth 12 vs 8.56e8 at 72 us for
  // 256-row items on 128 workgroups at depth 16; LR 256-row items (8.47e8 at 56 us; 512:
  // 7.3e8) -- profiles/r2/persist_full_item/
  // G32 ensembles far beyond BASELINE's 100 x 6 (> 1200 tree levels a row) are VALU-bound:
  // 256-row items on 512 workgroups spread them over more waves (700 x 6 at depth 6:
  // 1.01e9 tx/s vs 7.3e8 with 512-row items on 256, profiles/r2/g32_large_ensembles/)
  pl.big_trees = g32 && gbdt_trees * gbdt_depth > 1200;
  pl.item_rows = pl.big_trees ? 256 : (g32 || (w64 && model == CCFD_MODEL_MLP)) ? 512 : CCFD_PERSIST_ITEM_ROWS;
  if (env_rows == 256 || env_rows == 512 || env_rows == 1024 || (!g32 && (env_rows == 64 || env_rows == 128)))
    pl.item_rows = env_rows;
  pl.tiles_per_wave = g32 ? pl.item_rows / 256 : pl.item_rows / 64;
  // Pipelined static items (MLP on W64 rows, score_persist.hip persist_pipe_kernel): a
  // micro-batch spread over 32 workgroups / CUs, the next item's rows fetched while the
  // current one is scored -- 19 us unloaded latency vs 29 us for claimed 512-row items,
  // better up to ~4 batches in flight, capped near 6.5e8 tx/s beyond
  // (profiles/r3/latency/).  persist_items: 2 = pipelined, 1 = claimed, 0 = env
  // CCFD_PERSIST_PIPE (default claimed).  CCFD_PERSIST_ITEM_ROWS = 64 / 128 (default 128).
  // GBDT on G32 / G20 rows: the same pipelined static items, 512-row items, leaves in LDS
  // (score_gbdt_g32_persist.hip persist_gbdt_pipe_kernel)
  const bool g32_pipe_ok = g32 && !pl.big_trees && ((long)gbdt_trees << gbdt_depth) <= 16384;   // kG32LeafLds
  if ((w64 && model == CCFD_MODEL_MLP) || g32_pipe_ok) {
    if (persist_items == 2) pl.pipe = true;
    else if (persist_items == 0 && env_pipe) pl.pipe = std::atoi(env_pipe) != 0;
  }
  if (pl.pipe && g32) {
    pl.item_rows = 512;
    pl.tiles_per_wave = 2;
  } else if (pl.pipe) {
    pl.item_rows = env_rows == 64 ? 64 : 128;
    pl.tiles_per_wave = pl.item_rows / 64;
  }
  pl.items_per_batch = (max_batch + pl.item_rows - 1) / pl.item_rows;
  // resident workgroups (+ the doorbell): 128 for GBDT G32 (1.68e9 tx/s vs 1.62e9 at 256 and
  // 1.34e9 at 768, profiles/r2/gbdt_g32_persist_sweep.jsonl) and f32 rows; 64 for W64 rows
  // (their 512-row items keep 32 KB per workgroup in flight)
  // G32 ensembles well beyond BASELINE's 100 x 6 are VALU-bound, not PCIe-bound: two
  // workgroups per CU (700 x 6: 3.8e8 tx/s at 128, 7.3e8 at 256 and 1.01e9 at 512 with
  // 256-row items, profiles/r2/g32_large_ensembles/)
  // G20 rows carry 1.6x the rows of G32 per PCIe byte, so more resident workgroups keep
  // up: 216 (2.56-2.57e9 tx/s at p50 91 us, depth 4, 512-row items) vs 2.52e9 at 192,
  // 2.53e9 at 240 and 2.45e9 at 249 (profiles/r5/pass_w/; r2: 2.18e9 at 128, g20/sweep.txt)
  pl.grid = persist_grid > 0 ? persist_grid
            : pl.pipe ? CCFD_PERSIST_GRID
            : w64 ? CCFD_PERSIST_GRID_W64
            : pl.big_trees ? 4 * CCFD_PERSIST_GRID
            : wire == 3 ? CCFD_PERSIST_GRID_G20 : CCFD_PERSIST_GRID;
  return pl;
}

}  // namespace ccfd

// Table check of the persistent kernels' work plan (csrc/engine/persist_plan.h), built plain
// by tests/test_native_cpu.py.  Every row is the plan the engine is expected to choose for one
// configuration, written out as literals (ABI constants: 256-row default items, grids 128 /
// 64 W64 / 216 G20); each row is checked again with persist_grid = 37, which overrides the
// grid and nothing else.  Exit code 0 = every row matched.
#include <cstdio>

#include "../engine/persist_plan.h"

namespace {

struct Case {
  const char* name;
  int model, wire, trees, depth, max_batch, persist_items;
  const char* env_rows;
  const char* env_pipe;
  int item_rows, tiles_per_wave;
  bool pipe;
  int items_per_batch, grid;
  bool big_trees;
};

constexpr int LR = CCFD_MODEL_LR, MLP = CCFD_MODEL_MLP, GBDT = CCFD_MODEL_GBDT;
constexpr int F32 = 0, W64 = 1, G32 = 2, G20 = 3;

const Case kCases[] = {
    // name                                  model wire trees depth batch items rows   pipe    | item tpw pipe  C  grid big
    {"MLP f32",                              MLP,  F32, 0,   0, 4096, 0, nullptr, nullptr,  256,  4, false, 16, 128, false},
    {"MLP W64",                              MLP,  W64, 0,   0, 4096, 0, nullptr, nullptr,  512,  8, false,  8,  64, false},
    {"LR W64",                               LR,   W64, 0,   0, 4096, 0, nullptr, nullptr,  256,  4, false, 16,  64, false},
    {"MLP W64 persist_items=2",              MLP,  W64, 0,   0, 4096, 2, nullptr, nullptr,  128,  2, true,  32, 128, false},
    {"MLP W64 persist_items=2 ITEM_ROWS=64", MLP,  W64, 0,   0, 4096, 2, "64",    nullptr,   64,  1, true,  64, 128, false},
    {"MLP W64 persist_items=2 ITEM_ROWS=256", MLP, W64, 0,   0, 4096, 2, "256",   nullptr,  128,  2, true,  32, 128, false},
    {"MLP W64 persist_items=0 PIPE=1",       MLP,  W64, 0,   0, 4096, 0, nullptr, "1",      128,  2, true,  32, 128, false},
    {"MLP W64 persist_items=1 PIPE=1",       MLP,  W64, 0,   0, 4096, 1, nullptr, "1",      512,  8, false,  8,  64, false},
    {"LR W64 persist_items=2",               LR,   W64, 0,   0, 4096, 2, nullptr, nullptr,  256,  4, false, 16,  64, false},
    {"MLP f32 ITEM_ROWS=64",                 MLP,  F32, 0,   0, 4096, 0, "64",    nullptr,   64,  1, false, 64, 128, false},
    {"MLP f32 ITEM_ROWS=1024",               MLP,  F32, 0,   0, 4096, 0, "1024",  nullptr, 1024, 16, false,  4, 128, false},
    {"MLP f32 ITEM_ROWS=96",                 MLP,  F32, 0,   0, 4096, 0, "96",    nullptr,  256,  4, false, 16, 128, false},
    {"GBDT G32 100x6",                       GBDT, G32, 100, 6, 4096, 0, nullptr, nullptr,  512,  2, false,  8, 128, false},
    {"GBDT G20 100x6",                       GBDT, G20, 100, 6, 4096, 0, nullptr, nullptr,  512,  2, false,  8, 216, false},
    {"GBDT G20 100x6 persist_items=2",       GBDT, G20, 100, 6, 4096, 2, nullptr, nullptr,  512,  2, true,   8, 128, false},
    {"GBDT G32 100x6 ITEM_ROWS=128",         GBDT, G32, 100, 6, 4096, 0, "128",   nullptr,  512,  2, false,  8, 128, false},
    {"GBDT G32 100x6 ITEM_ROWS=1024",        GBDT, G32, 100, 6, 4096, 0, "1024",  nullptr, 1024,  4, false,  4, 128, false},
    {"GBDT G32 200x6 persist_items=2",       GBDT, G32, 200, 6, 4096, 2, nullptr, nullptr,  512,  2, true,   8, 128, false},   // 1200 levels: not big; 12800 leaves
    {"GBDT G32 100x8 persist_items=2",       GBDT, G32, 100, 8, 4096, 2, nullptr, nullptr,  512,  2, false,  8, 128, false},   // 25600 leaves: no pipe
    {"GBDT G32 700x6",                       GBDT, G32, 700, 6, 4096, 0, nullptr, nullptr,  256,  1, false, 16, 512, true},
    {"GBDT G20 700x6",                       GBDT, G20, 700, 6, 4096, 0, nullptr, nullptr,  256,  1, false, 16, 512, true},
    {"GBDT G32 700x6 persist_items=2",       GBDT, G32, 700, 6, 4096, 2, nullptr, nullptr,  256,  1, false, 16, 512, true},
    {"GBDT G32 201x6",                       GBDT, G32, 201, 6, 4096, 0, nullptr, nullptr,  256,  1, false, 16, 512, true},    // 1206 levels: big
    {"MLP W64 max_batch=1000",               MLP,  W64, 0,   0, 1000, 0, nullptr, nullptr,  512,  8, false,  2,  64, false},
};

int check(const Case& c, int persist_grid) {
  const ccfd::PersistPlan p = ccfd::persist_plan(c.model, c.wire, c.trees, c.depth, c.max_batch, c.persist_items,
                                                 persist_grid, c.env_rows, c.env_pipe);
  const int grid = persist_grid > 0 ? persist_grid : c.grid;
  if (p.item_rows == c.item_rows && p.tiles_per_wave == c.tiles_per_wave && p.pipe == c.pipe &&
      p.items_per_batch == c.items_per_batch && p.grid == grid && p.big_trees == c.big_trees)
    return 0;
  std::fprintf(stderr, "%s (persist_grid %d): got {%d, %d, %d, %d, %d, %d}, want {%d, %d, %d, %d, %d, %d}\n", c.name,
               persist_grid, p.item_rows, p.tiles_per_wave, (int)p.pipe, p.items_per_batch, p.grid, (int)p.big_trees,
               c.item_rows, c.tiles_per_wave, (int)c.pipe, c.items_per_batch, grid, (int)c.big_trees);
  return 1;
}

}  // namespace

int main() {
  int fail = 0, n = 0;
  for (const Case& c : kCases) {
    fail += check(c, 0);
    fail += check(c, 37);
    ++n;
  }
  if (fail) { std::fprintf(stderr, "persist plan check FAILED (%d)\n", fail); return 1; }
  std::printf("persist plan check ok: %d cases\n", n);
  return 0;
}

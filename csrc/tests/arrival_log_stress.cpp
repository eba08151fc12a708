// Stress test of the engine's per-partition arrival log (csrc/engine/arrival_log.h), built by
// tests/test_native_cpu.py with -fsanitize=thread.  A committer thread pushes heads that grow
// by 1..64 and then publishes the head, as ring_commit() does; a reader asks arrival_of(row)
// for rows below the last published head and forgets entries behind itself.  Every answer is
// the entry with the smallest recorded head greater than the row.  Exit code 0 = all held.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <vector>

#include "../engine/arrival_log.h"

namespace {
int64_t time_of(int64_t head) { return head * 3 + 1; }
int64_t origin_of(int64_t head) { return head ^ 0x5555; }
}  // namespace

int main(int argc, char** argv) {
  const int n = argc > 1 ? std::atoi(argv[1]) : 200000;
  std::vector<int64_t> heads(n);                       // the commit sequence, fixed up front
  {
    std::mt19937_64 rng(3);
    int64_t h = 0;
    for (int i = 0; i < n; ++i) heads[i] = h += 1 + (int64_t)(rng() % 64);
  }
  ccfd::ArrivalLog log;
  {
    const ccfd::ArrivalLog::Arrival a = log.arrival_of(0);
    if (a.head != 0 || a.t != 0 || a.origin != 0) { std::fprintf(stderr, "empty log: not {0,0,0}\n"); return 1; }
  }
  std::atomic<int64_t> published{0};
  std::atomic<bool> failed{false};

  std::thread committer([&] {
    std::mt19937_64 rng(4);
    for (int i = 0; i < n && !failed.load(); ++i) {
      log.push(heads[i], time_of(heads[i]), origin_of(heads[i]));      // stamp first
      published.store(heads[i], std::memory_order_release);              // then publish
      if (rng() % 256 == 0) std::this_thread::sleep_for(std::chrono::microseconds(rng() % 30));
    }
  });

  std::thread reader([&] {
    std::mt19937_64 rng(5);
    int64_t low = 0;                                   // rows below it are forgotten
    uint64_t asked = 0;
    while (!failed.load()) {
      const int64_t h = published.load(std::memory_order_acquire);
      if (h > low) {
        const int64_t row = low + (int64_t)(rng() % (uint64_t)(h - low));
        const ccfd::ArrivalLog::Arrival a = log.arrival_of(row);
        const int64_t want = *std::upper_bound(heads.begin(), heads.end(), row);
        if (a.head != want || a.t != time_of(want) || a.origin != origin_of(want)) {
          std::fprintf(stderr, "row %lld: got head %lld, want %lld\n", (long long)row, (long long)a.head, (long long)want);
          failed.store(true);
          return;
        }
        ++asked;
        if (rng() % 4 == 0) {                          // release some rows behind this one
          low += (int64_t)(rng() % (uint64_t)(row - low + 1));
          log.forget_before(low);
        }
      }
      if (h == heads.back() && (low >= h - 64 || asked > 4u * (uint64_t)heads.size())) return;
    }
  });

  committer.join();
  reader.join();
  if (!failed.load()) {
    // past the newest head: the newest entry; everything forgotten: {0,0,0} again
    const ccfd::ArrivalLog::Arrival a = log.arrival_of(heads.back() + 5);
    if (a.head != heads.back()) { std::fprintf(stderr, "row past the newest head: got %lld\n", (long long)a.head); failed.store(true); }
    log.forget_before(heads.back());
    if (log.arrival_of(0).head != 0) { std::fprintf(stderr, "emptied log: not {0,0,0}\n"); failed.store(true); }
  }
  if (failed.load()) { std::fprintf(stderr, "arrival log stress FAILED\n"); return 1; }
  std::printf("arrival log stress ok: %d commits\n", n);
  return 0;
}

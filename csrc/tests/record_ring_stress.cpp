// Stress test of the engine's record ring (csrc/engine/record_ring.h), built by
// tests/test_native_cpu.py with -fsanitize=thread and with address,undefined.
//
// Phase 1 (the flagged ring's contract): one producer pushes batches of 0..700 numbered
// records and, like the engine's complete(), waits until room() covers the whole batch first;
// two drainers pull with random `max` and random sleeps.  Every number is drained exactly
// once, each drainer sees increasing numbers, nothing is dropped.
// Phase 2 (the scored ring's contract): the producer never waits.  It either offers every
// record (next() refuses and counts what does not fit) or takes what fits and drops the rest
// up front.  Accepted + dropped = pushed, and exactly the accepted records come out: an
// unread record is never overwritten.  Exit code 0 = all held.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <vector>

#include "../engine/record_ring.h"

namespace {

struct Rec { uint64_t no; uint64_t twin; };   // twin = ~no: a torn or stale record shows

struct Drained { std::vector<uint64_t> nos; bool ok = true; };

void drainer(ccfd::RecordRing<Rec>& ring, std::atomic<bool>& done, uint64_t seed, Drained* out) {
  std::mt19937_64 rng(seed);
  std::vector<Rec> buf(900);
  for (;;) {
    const bool last = done.load(std::memory_order_acquire);      // read before the drain
    const int64_t k = ring.drain(buf.data(), (int64_t)(rng() % 900));
    for (int64_t i = 0; i < k; ++i) {
      if (buf[i].twin != ~buf[i].no || (!out->nos.empty() && buf[i].no <= out->nos.back())) out->ok = false;
      out->nos.push_back(buf[i].no);
    }
    if (last && k == 0 && ring.room() == 1021) return;
    if (rng() % 16 == 0) std::this_thread::sleep_for(std::chrono::microseconds(rng() % 40));
  }
}

// runs one phase; returns false on any violated property
bool phase(bool check_room, uint64_t total) {
  ccfd::RecordRing<Rec> ring;
  ring.reset(1021);                                   // prime: wraps at odd offsets
  std::atomic<bool> done{false};
  Drained d[2];
  std::thread t0(drainer, std::ref(ring), std::ref(done), 11, &d[0]);
  std::thread t1(drainer, std::ref(ring), std::ref(done), 12, &d[1]);

  std::mt19937_64 rng(check_room ? 1 : 2);
  std::vector<char> accepted(total, 0);
  uint64_t next = 0, n_accepted = 0;
  while (next < total) {
    const uint64_t n = std::min<uint64_t>(rng() % 701, total - next);
    if (check_room)
      while (ring.room() < n) std::this_thread::yield();
    {
      auto w = ring.writer();
      uint64_t offer = n;
      if (!check_room && rng() % 2) {                 // take what fits, drop the remainder
        offer = std::min<uint64_t>(w.room(), n);
        w.drop(n - offer);
      }
      for (uint64_t i = 0; i < n; ++i) {
        if (i >= offer) continue;
        if (Rec* r = w.next()) {
          r->no = next + i;
          r->twin = ~(next + i);
          accepted[next + i] = 1;
          ++n_accepted;
        }
      }
    }
    next += n;
    if (rng() % 32 == 0) std::this_thread::sleep_for(std::chrono::microseconds(rng() % 30));
  }
  done.store(true, std::memory_order_release);
  t0.join();
  t1.join();

  bool ok = d[0].ok && d[1].ok;
  if (!ok) std::fprintf(stderr, "a drainer saw a torn or out-of-order record\n");
  std::vector<char> seen(total, 0);
  for (const Drained& dr : d)
    for (uint64_t no : dr.nos) {
      if (no >= total || seen[no]) { std::fprintf(stderr, "record %llu drained twice\n", (unsigned long long)no); ok = false; }
      else seen[no] = 1;
    }
  for (uint64_t i = 0; i < total; ++i)
    if (seen[i] != accepted[i]) { std::fprintf(stderr, "record %llu: accepted %d drained %d\n", (unsigned long long)i, accepted[i], seen[i]); ok = false; break; }
  const uint64_t dropped = ring.dropped();
  if (n_accepted + dropped != total) { std::fprintf(stderr, "accepted %llu + dropped %llu != pushed %llu\n", (unsigned long long)n_accepted, (unsigned long long)dropped, (unsigned long long)total); ok = false; }
  if (check_room && dropped != 0) { std::fprintf(stderr, "dropped %llu with room reserved\n", (unsigned long long)dropped); ok = false; }
  if (!check_room && dropped == 0) { std::fprintf(stderr, "phase 2 never filled the ring\n"); ok = false; }
  return ok;
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t total = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 400000;
  if (!phase(true, total) || !phase(false, total)) { std::fprintf(stderr, "record ring stress FAILED\n"); return 1; }
  std::printf("record ring stress ok: 2 x %llu records through a 1021-record ring\n", (unsigned long long)total);
  return 0;
}

// Stress test of the engine's completion stamper (csrc/engine/completion_stamper.h), built by
// tests/test_native_cpu.py with -fsanitize=thread.  8 slots; a "device" thread publishes the
// awaited sequence number into a slot's completion record after a random delay; the owner
// thread arms a slot, waits for its record, asks landed_ns() and re-arms with the next
// sequence number, 20000 times.  Slot 7's sequence numbers differ by 65536 (the same 16-bit
// tag every time) and it is reused at once, so after its first use the stamper's word is
// always a stale one: it must be rejected, never accepted with a time before the submit.
// The stamper is destroyed while every slot is armed.  Exit code 0 = all held.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <random>
#include <thread>

#include "../engine/completion_stamper.h"

namespace {

constexpr int kSlots = 8;
constexpr int kRounds = 20000;

alignas(64) unsigned long long g_rec[kSlots][8];      // completion records: [0] = sequence
std::atomic<unsigned long long> g_want[kSlots];        // owner -> device: publish this
int64_t g_pub_ns[kSlots];                              // device: time just before it published

void device(std::atomic<bool>& stop) {
  std::mt19937_64 rng(5);
  unsigned long long done[kSlots] = {};
  while (!stop.load(std::memory_order_relaxed)) {
    for (int i = 0; i < kSlots; ++i) {
      const unsigned long long w = g_want[i].load(std::memory_order_acquire);
      if (w == done[i]) continue;
      if (i != kSlots - 1) {                           // the last slot completes at once
        const int64_t until = ccfd::now_ns() + (int64_t)(rng() % 8000);
        while (ccfd::now_ns() < until) ccfd::cpu_relax();
        if (rng() % 256 == 0) std::this_thread::sleep_for(std::chrono::microseconds(rng() % 60));
      }
      g_pub_ns[i] = ccfd::now_ns();
      __atomic_store_n(&g_rec[i][0], w, __ATOMIC_RELEASE);
      done[i] = w;
    }
  }
}

}  // namespace

int main() {
  int fail = 0;
  std::atomic<bool> stop{false};
  std::thread dev(device, std::ref(stop));
  uint64_t calls = 0, accepted = 0, accepted_last = 0, used = 0, missed = 0, rejected = 0;
  {
    ccfd::CompletionStamper st;
    st.start(kSlots);
    std::mt19937_64 rng(6);
    unsigned long long expect[kSlots] = {};
    int64_t t_submit[kSlots] = {};
    auto submit = [&](int i) {
      expect[i] = expect[i] ? expect[i] + (i == kSlots - 1 ? 65536 : kSlots) : (unsigned long long)(i + 1);
      t_submit[i] = ccfd::now_ns();
      st.arm((size_t)i, g_rec[i], expect[i]);
      g_want[i].store(expect[i], std::memory_order_release);
    };
    for (int it = 0; it < kRounds && !fail; ++it) {
      const int i = it % kSlots;
      if (expect[i]) {
        while (__atomic_load_n(&g_rec[i][0], __ATOMIC_ACQUIRE) != expect[i]) ccfd::cpu_relax();
        if (rng() % 4 == 0) {                          // the owner looks late: the stamp matters
          const int64_t until = ccfd::now_ns() + (int64_t)(rng() % 20000);
          while (ccfd::now_ns() < until) ccfd::cpu_relax();
        }
        const int64_t fallback = ccfd::now_ns();
        const uint64_t used0 = st.used;
        const int64_t t = st.landed_ns((size_t)i, expect[i], t_submit[i], fallback);
        ++calls;
        if (st.used != used0) {
          ++accepted;
          accepted_last += i == kSlots - 1;
          // inside the batch's life, and not from before this sequence number was published:
          // a stamp taken for another use of the slot would be older
          if (t < t_submit[i] || t > fallback || t < g_pub_ns[i]) {
            std::fprintf(stderr, "slot %d seq %llu: stamp %lld outside [submit %lld, published %lld, seen %lld]\n", i,
                         expect[i], (long long)t, (long long)t_submit[i], (long long)g_pub_ns[i], (long long)fallback);
            ++fail;
          }
        } else if (t != fallback) {
          std::fprintf(stderr, "slot %d: a stamp that was not accepted was returned\n", i);
          ++fail;
        }
      }
      submit(i);
    }
    used = st.used; missed = st.missed; rejected = st.rejected;
    // every slot is armed (the last kSlots submissions were never collected): the destructor
    // joins the thread all the same
  }
  stop.store(true);
  dev.join();
  if (used != accepted || used + missed + rejected != calls) {
    std::fprintf(stderr, "used %llu + missed %llu + rejected %llu != %llu calls\n", (unsigned long long)used,
                 (unsigned long long)missed, (unsigned long long)rejected, (unsigned long long)calls);
    ++fail;
  }
  if (used == 0) { std::fprintf(stderr, "no stamp was ever used\n"); ++fail; }
  // slot 7: its first use can be stamped; every later word carries the same tag and is stale
  if (accepted_last > 1) { std::fprintf(stderr, "slot 7 accepted %llu stamps\n", (unsigned long long)accepted_last); ++fail; }
  if (fail) { std::fprintf(stderr, "stamper stress FAILED\n"); return 1; }
  std::printf("stamper stress ok: %llu calls, %llu used, %llu missed, %llu rejected\n", (unsigned long long)calls,
              (unsigned long long)used, (unsigned long long)missed, (unsigned long long)rejected);
  return 0;
}

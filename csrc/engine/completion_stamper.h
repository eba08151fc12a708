// Completion stamper (CCFD_COMPLETION_THREAD, default on): a host thread that watches the
// kernel-published completion records of the in-flight micro-batches and stamps the host
// time each one lands, so a batch's latency ends when its results are in host memory, not
// when the pump thread next looks (between pump() calls the caller runs the router
// hand-off and the X2 tick: without the stamper those milliseconds were charged to every
// batch that completed meanwhile -- the p99 tail).  One packed word per slot: the low 16
// bits of the awaited sequence number << 48 | ns since start (48 bits), so a stamp can
// never be attributed to another use of the slot.
//
// A completion record is only ever seen as `const volatile unsigned long long*` whose first
// word becomes the awaited sequence number.  Header-only and HIP-free:
// csrc/tests/stamper_stress.cpp runs it under ThreadSanitizer (tests/test_native_cpu.py).
// arm() / landed_ns() belong to one owner thread.
#pragma once
#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <thread>

#include <sys/prctl.h>

#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace ccfd {

inline int64_t now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(
             std::chrono::steady_clock::now().time_since_epoch()).count();
}

inline void cpu_relax() {
#if defined(__x86_64__)
  _mm_pause();
#endif
}

class CompletionStamper {
 public:
  using Record = const volatile unsigned long long*;

  // CCFD_STAMPER_DEBUG report
  uint64_t used = 0, missed = 0, rejected = 0;
  std::atomic<uint64_t> written{0}, iters{0};

  CompletionStamper() = default;
  CompletionStamper(const CompletionStamper&) = delete;
  CompletionStamper& operator=(const CompletionStamper&) = delete;
  ~CompletionStamper() { stop(); }

  bool on() const { return th_.joinable(); }

  void start(size_t n_slots) {
    n_ = n_slots;
    armed_.reset(new std::atomic<unsigned long long>[n_]);
    ptr_.reset(new std::atomic<Record>[n_]);
    word_.reset(new std::atomic<uint64_t>[n_]);
    for (size_t i = 0; i < n_; ++i) { armed_[i] = 0; ptr_[i] = nullptr; word_[i] = 0; }
    base_ns_ = now_ns();
    stop_.store(false);
    th_ = std::thread([this] { loop(); });
  }

  // joins the thread (slots may still be armed); the records may be freed afterwards
  void stop() {
    stop_.store(true);
    if (th_.joinable()) th_.join();
  }

  // slot `i` now awaits `expect` in rec[0]
  void arm(size_t i, Record rec, unsigned long long expect) {
    if (!on()) return;
    ptr_[i].store(rec, std::memory_order_relaxed);
    armed_[i].store(expect, std::memory_order_release);
  }

  // Host time the record of slot `i` (armed for `expect`, submitted at `t_submit`) landed,
  // else `fallback` (the time the owner saw it); disarms the slot.  A word of another
  // sequence number is a miss; a time after the fallback or before the submit is rejected.
  int64_t landed_ns(size_t i, unsigned long long expect, int64_t t_submit, int64_t fallback) {
    if (!on()) return fallback;
    const uint64_t w = word_[i].load(std::memory_order_acquire);
    armed_[i].store(0, std::memory_order_relaxed);
    if ((w >> 48) != (expect & 0xffffull)) { ++missed; return fallback; }
    const int64_t t = base_ns_ + (int64_t)(w & kStampMask);
    if (t <= fallback && t >= t_submit) { ++used; return t; }
    ++rejected;
    return fallback;
  }

 private:
  static constexpr uint64_t kStampMask = (1ull << 48) - 1;

  void loop() {
    prctl(PR_SET_TIMERSLACK, 1000UL, 0, 0, 0);
    while (!stop_.load(std::memory_order_relaxed)) {
      bool any = false;
      for (size_t i = 0; i < n_; ++i) {
        const unsigned long long e = armed_[i].load(std::memory_order_acquire);
        if (!e) continue;
        any = true;
        const uint64_t tag = (uint64_t)(e & 0xffffull) << 48;
        if ((word_[i].load(std::memory_order_relaxed) & ~kStampMask) == tag) continue;   // stamped
        Record p = ptr_[i].load(std::memory_order_relaxed);
        if (p && __atomic_load_n(p, __ATOMIC_RELAXED) == e) {
          word_[i].store(tag | ((uint64_t)(now_ns() - base_ns_) & kStampMask), std::memory_order_release);
          written.fetch_add(1, std::memory_order_relaxed);
        }
      }
      iters.fetch_add(1, std::memory_order_relaxed);
      if (any) cpu_relax();
      else std::this_thread::sleep_for(std::chrono::microseconds(2));
    }
  }

  size_t n_ = 0;
  int64_t base_ns_ = 0;
  std::unique_ptr<std::atomic<unsigned long long>[]> armed_;   // awaited seq (0 = idle)
  std::unique_ptr<std::atomic<Record>[]> ptr_;
  std::unique_ptr<std::atomic<uint64_t>[]> word_;              // tag << 48 | t
  std::thread th_;
  std::atomic<bool> stop_{false};
};

}  // namespace ccfd

// Arrival log of one ring partition: for every producer commit, the ring head after it, the
// commit time and the producer's send time.  The ingest thread pushes (before it publishes the
// rows, so a row the consumer can see always has its entry); the engine thread looks up the
// entry that covers a micro-batch's first row and forgets entries behind the released rows.
// Header-only and HIP-free: csrc/tests/arrival_log_stress.cpp runs it under ThreadSanitizer
// (tests/test_native_cpu.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <deque>
#include <mutex>

namespace ccfd {

class ArrivalLog {
 public:
  struct Arrival { int64_t head, t, origin; };       // head after commit, commit time, producer send time

  // heads must increase from push to push
  void push(int64_t head, int64_t t, int64_t origin) {
    std::lock_guard<std::mutex> lk(mu_);
    log_.push_back(Arrival{head, t, origin});
  }

  // commit (and origin) time of `row`: the entry with the smallest head > row; the newest
  // entry when there is none, {0, 0, 0} when the log is empty
  Arrival arrival_of(int64_t row) {
    std::lock_guard<std::mutex> lk(mu_);
    // heads increase monotonically: binary search (a JSON feed commits one entry per message,
    // so tens of thousands of entries are in flight and a linear scan held the mutex -- and the
    // ingest thread's next commit -- for tens of microseconds)
    auto it = std::upper_bound(log_.begin(), log_.end(), row,
                               [](int64_t r, const Arrival& a) { return r < a.head; });
    if (it != log_.end()) return *it;
    return log_.empty() ? Arrival{0, 0, 0} : log_.back();
  }

  // drop the entries whose rows are all below `row`
  void forget_before(int64_t row) {
    std::lock_guard<std::mutex> lk(mu_);
    while (!log_.empty() && log_.front().head <= row) log_.pop_front();
  }

 private:
  std::mutex mu_;
  std::deque<Arrival> log_;
};

}  // namespace ccfd

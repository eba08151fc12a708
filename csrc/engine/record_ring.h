// Mutex-guarded record ring between the engine's completion path (one producer) and any
// number of drainer threads.  The flagged hand-off ring and the opt-in scored-record ring are
// two instances; unread records are never overwritten -- what does not fit is counted.
//
//   producer:  room() -> { auto w = ring.writer(); ... *w.next() = rec; ... }   (one lock a batch)
//   drainer:   drain(out, max)
//
// Only drainers free records, so room() can only have grown by the time the writer is taken:
// a producer that checks room() first never sees next() fail.
// Header-only and HIP-free: csrc/tests/record_ring_stress.cpp runs it under ThreadSanitizer
// and ASan/UBSan (tests/test_native_cpu.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

namespace ccfd {

template <class T>
class RecordRing {
 public:
  // empty ring of `capacity` records; the dropped count restarts
  void reset(size_t capacity) {
    std::lock_guard<std::mutex> lk(mu_);
    buf_.assign(capacity, T{});
    head_ = tail_ = dropped_ = 0;
  }

  uint64_t room() {
    std::lock_guard<std::mutex> lk(mu_);
    return buf_.size() - (tail_ - head_);
  }

  uint64_t dropped() {
    std::lock_guard<std::mutex> lk(mu_);
    return dropped_;
  }

  int64_t drain(T* out, int64_t max) {
    std::lock_guard<std::mutex> lk(mu_);
    const uint64_t cap = buf_.size();
    int64_t k = 0;
    while (head_ < tail_ && k < max) out[k++] = buf_[head_++ % cap];
    return k;
  }

  // Batch push: holds the ring's lock for its lifetime.  It works on its own copy of the
  // ring's counters (nobody else can move them meanwhile) and puts them back at the end, so a
  // push loop keeps them in registers and pays one division a batch, not one a record.
  class Writer {
   public:
    explicit Writer(RecordRing& r)
        : r_(r), lk_(r.mu_), buf_(r.buf_.data()), cap_(r.buf_.size()), left_(cap_ - (r.tail_ - r.head_)),
          pos_(cap_ ? r.tail_ % cap_ : 0) {}
    ~Writer() {
      r_.tail_ += pushed_;
      r_.dropped_ += dropped_;
    }
    uint64_t room() const { return left_; }
    // the next record to fill, or nullptr (counted as dropped) when the ring is full
    T* next() {
      if (left_ == 0) { ++dropped_; return nullptr; }
      T* rec = buf_ + pos_;
      if (++pos_ == cap_) pos_ = 0;
      --left_;
      ++pushed_;
      return rec;
    }
    // records the producer gives up on without offering them
    void drop(uint64_t n) { dropped_ += n; }

   private:
    RecordRing& r_;
    std::lock_guard<std::mutex> lk_;
    T* const buf_;
    const uint64_t cap_;
    uint64_t left_, pos_, pushed_ = 0, dropped_ = 0;
  };
  Writer writer() { return Writer(*this); }

 private:
  std::vector<T> buf_;
  uint64_t head_ = 0, tail_ = 0, dropped_ = 0;
  std::mutex mu_;
};

}  // namespace ccfd

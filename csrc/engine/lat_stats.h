// Per-batch latency statistics of the streaming engine: O(1) memory however long the engine
// runs (a long-lived service scores ~2e5 batches/s).
//
//   LogHist       256 buckets, 4 per octave of ns (bucket i holds [2^(i/4), 2^((i+1)/4))), with
//                 a row-weighted twin (each batch adds its row count: the per-transaction
//                 distributions exported as the Seldon request histograms); merged over ranks (X3)
//   LatencyStats  count / sum / max, a 0.25-us linear histogram up to 4 ms for the reported
//                 quantiles, three LogHists (end-to-end, device window, producer send -> scored)
//                 and the host time counters of the submission / completion thread
//
// Header-only and HIP-free: csrc/tests/lat_stats_check.cpp runs it under ASan/UBSan
// (tests/test_native_cpu.py).  Not thread-safe: the engine touches it under its API lock.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../include/ccfd_abi.h"

namespace ccfd {

struct LogHist {
  uint64_t batches[256] = {};
  uint64_t rows[256] = {};

  // below 1 ns -> bucket 0, beyond the last octave -> 255
  static int log_bucket(double ns) {
    return ns < 1.0 ? 0 : std::min(255, (int)std::floor(4.0 * std::log2(ns)));
  }
  void add(double ns, uint64_t n_rows) {
    const int b = log_bucket(ns);
    ++batches[b];
    rows[b] += n_rows;
  }
  void clear() {
    std::memset(batches, 0, sizeof(batches));
    std::memset(rows, 0, sizeof(rows));
  }
};

class LatencyStats {
 public:
  static constexpr int kFineBuckets = 16384;
  static constexpr double kFineUs = 0.25;

  uint64_t lat_n = 0, lat_over = 0;
  double lat_sum_us = 0.0, lat_max_us = 0.0;
  std::vector<uint64_t> lat_fine = std::vector<uint64_t>(kFineBuckets, 0u);   // u64: never wraps
  LogHist lat, dev, origin;
  uint64_t origin_batches = 0;
  uint64_t dev_batches = 0, dev_exec_ns = 0;
  uint64_t host_submit_ns = 0, host_wait_ns = 0, host_complete_ns = 0;

  // one completed batch: `ns` from arrival (or submit) to its results in host memory,
  // `origin_ns` from the producer's send time to the same point (<= 0: unknown)
  void record(int64_t ns, int64_t origin_ns, uint64_t rows) {
    const double us = ns * 1e-3;
    ++lat_n;
    lat_sum_us += us;
    lat_max_us = std::max(lat_max_us, us);
    const double fb = us / kFineUs;
    if (fb < kFineBuckets) ++lat_fine[(size_t)fb]; else ++lat_over;
    lat.add((double)ns, rows);
    if (origin_ns > 0) {
      ++origin_batches;
      origin.add((double)origin_ns, rows);
    }
  }

  // K7: device-clock execution window of one batch
  void record_device(double ns, uint64_t rows) {
    dev_exec_ns += (uint64_t)ns;
    ++dev_batches;
    dev.add(ns, rows);
  }

  // nearest-rank quantile from the fine histogram (bucket midpoint); samples beyond its
  // range report the max
  double fine_quantile(double q) const {
    const uint64_t k = (uint64_t)std::floor(q * (double)(lat_n - 1) + 0.5);
    uint64_t c = 0;
    for (int i = 0; i < kFineBuckets; ++i) {
      c += lat_fine[i];
      if (c > k) return (i + 0.5) * kFineUs;
    }
    return lat_max_us;
  }

  // end-to-end and origin latency only: the device histograms and host time counters stay
  void reset_latency() {
    lat_n = lat_over = 0;
    lat_sum_us = lat_max_us = 0.0;
    std::fill(lat_fine.begin(), lat_fine.end(), 0ull);
    lat.clear();
    origin_batches = 0;
    origin.clear();
  }

  // ccfd_engine_reset_stats
  void reset_all() {
    reset_latency();
    host_submit_ns = host_wait_ns = host_complete_ns = 0;
    dev_batches = dev_exec_ns = 0;
    dev.clear();
  }

  // the four quantile fields are left as they are until a batch has completed
  void fill(ccfd_engine_stats* st) const {
    std::memcpy(st->lat_hist, lat.batches, sizeof(st->lat_hist));
    std::memcpy(st->lat_hist_rows, lat.rows, sizeof(st->lat_hist_rows));
    st->host_submit_ns = host_submit_ns;
    st->host_wait_ns = host_wait_ns;
    st->host_complete_ns = host_complete_ns;
    st->dev_batches = dev_batches;
    st->dev_exec_ns = dev_exec_ns;
    std::memcpy(st->dev_hist, dev.batches, sizeof(st->dev_hist));
    std::memcpy(st->dev_hist_rows, dev.rows, sizeof(st->dev_hist_rows));
    st->origin_batches = origin_batches;
    std::memcpy(st->origin_hist, origin.batches, sizeof(st->origin_hist));
    std::memcpy(st->origin_hist_rows, origin.rows, sizeof(st->origin_hist_rows));
    if (lat_n == 0) return;
    st->lat_p50_us = fine_quantile(0.50);
    st->lat_p99_us = fine_quantile(0.99);
    st->lat_max_us = lat_max_us;
    st->lat_mean_us = lat_sum_us / (double)lat_n;
  }
};

}  // namespace ccfd

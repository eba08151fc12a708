// Checks of the engine's latency statistics (csrc/engine/lat_stats.h), built by
// tests/test_native_cpu.py with -fsanitize=address,undefined: the log-histogram bucket rule and
// its row-weighted twin, the nearest-rank quantiles of the fine histogram against the rule
// computed here from a sorted copy, the over-range and single-sample cases, and that each of
// the two resets clears exactly its own fields.  Exit code 0 = all held.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../engine/lat_stats.h"

namespace {

int g_fail = 0;
#define CHECK(c)                                                              \
  do {                                                                        \
    if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); ++g_fail; } \
  } while (0)

// the documented rule: nearest rank k = floor(q*(n-1)+0.5) of the sorted samples, reported as
// the midpoint of its 0.25-us bucket; at or beyond 4096 us the maximum
double rule_quantile(std::vector<int64_t> ns, double q) {
  std::sort(ns.begin(), ns.end());
  const size_t k = (size_t)std::floor(q * (double)(ns.size() - 1) + 0.5);
  const double us = ns[k] * 1e-3;
  if (us >= 4096.0) return ns.back() * 1e-3;
  return (std::floor(us / 0.25) + 0.5) * 0.25;
}

bool all_zero(const uint64_t* a) {
  for (int i = 0; i < 256; ++i) if (a[i]) return false;
  return true;
}

// every field carries something
void fill_everything(ccfd::LatencyStats& s) {
  s.record(12'345, 99'000, 7);
  s.record(5'000'000'000ll, 6'000'000'000ll, 3);     // beyond the fine histogram
  s.record_device(4'321.0, 7);
  s.host_submit_ns = 11;
  s.host_wait_ns = 22;
  s.host_complete_ns = 33;
}

struct Cleared { bool latency, device_and_host; };

void check_state(const ccfd::LatencyStats& s, Cleared c) {
  uint64_t fine = 0;
  for (uint64_t v : s.lat_fine) fine += v;
  // end-to-end and origin
  CHECK(s.lat_n == (c.latency ? 0u : 2u));
  CHECK(s.lat_over == (c.latency ? 0u : 1u));
  CHECK((s.lat_sum_us == 0.0) == c.latency);
  CHECK((s.lat_max_us == 0.0) == c.latency);
  CHECK(fine == (c.latency ? 0u : 1u));
  CHECK(all_zero(s.lat.batches) == c.latency);
  CHECK(all_zero(s.lat.rows) == c.latency);
  CHECK(s.origin_batches == (c.latency ? 0u : 2u));
  CHECK(all_zero(s.origin.batches) == c.latency);
  CHECK(all_zero(s.origin.rows) == c.latency);
  // device window and host time counters
  CHECK(s.dev_batches == (c.device_and_host ? 0u : 1u));
  CHECK(s.dev_exec_ns == (c.device_and_host ? 0u : 4321u));
  CHECK(all_zero(s.dev.batches) == c.device_and_host);
  CHECK(all_zero(s.dev.rows) == c.device_and_host);
  CHECK(s.host_submit_ns == (c.device_and_host ? 0u : 11u));
  CHECK(s.host_wait_ns == (c.device_and_host ? 0u : 22u));
  CHECK(s.host_complete_ns == (c.device_and_host ? 0u : 33u));
}

}  // namespace

int main() {
  using ccfd::LatencyStats;
  using ccfd::LogHist;

  // bucket rule
  CHECK(LogHist::log_bucket(0.5) == 0);
  CHECK(LogHist::log_bucket(1) == 0);
  CHECK(LogHist::log_bucket(2) == 4);
  CHECK(LogHist::log_bucket(1000) == 39);
  CHECK(LogHist::log_bucket(1e30) == 255);
  CHECK(LogHist::log_bucket(0) == 0);
  CHECK(LogHist::log_bucket(-3) == 0);

  {  // row weighting
    LogHist h;
    h.add(1000, 17);
    h.add(1000, 5);
    h.add(2, 1);
    CHECK(h.batches[39] == 2 && h.rows[39] == 22);
    CHECK(h.batches[4] == 1 && h.rows[4] == 1);
    uint64_t nb = 0, nr = 0;
    for (int i = 0; i < 256; ++i) { nb += h.batches[i]; nr += h.rows[i]; }
    CHECK(nb == 3 && nr == 23);
    h.clear();
    CHECK(all_zero(h.batches) && all_zero(h.rows));
  }

  {  // quantiles of 0.1, 0.3, ..., 19.9 us, fed in a scrambled order
    LatencyStats s;
    std::vector<int64_t> ns;
    for (int i = 0; i < 100; ++i) ns.push_back(100 + 200 * ((i * 37) % 100));
    for (int64_t v : ns) s.record(v, 0, 4);
    CHECK(s.lat_n == 100 && s.lat_over == 0);
    CHECK(s.fine_quantile(0.50) == rule_quantile(ns, 0.50));
    CHECK(s.fine_quantile(0.99) == rule_quantile(ns, 0.99));
    CHECK(rule_quantile(ns, 0.50) == 10.125);          // rank 50 = 10.1 us -> bucket [10, 10.25)
    CHECK(rule_quantile(ns, 0.99) == 19.625);          // rank 98 = 19.7 us -> bucket [19.5, 19.75)
    ccfd_engine_stats st{};
    s.fill(&st);
    CHECK(st.lat_p50_us == 10.125 && st.lat_p99_us == 19.625);
    CHECK(st.lat_max_us == 19'900 * 1e-3 && std::fabs(st.lat_mean_us - 10.0) < 1e-9);
    CHECK(st.origin_batches == 0 && all_zero(st.origin_hist));
    uint64_t nb = 0, nr = 0;
    for (int i = 0; i < 256; ++i) { nb += st.lat_hist[i]; nr += st.lat_hist_rows[i]; }
    CHECK(nb == 100 && nr == 400);
  }

  {  // 3 of 100 samples at or beyond 4096 us: p99 (rank 98) is the maximum
    LatencyStats s;
    std::vector<int64_t> ns;
    for (int i = 0; i < 97; ++i) ns.push_back(1000 + 10 * i);
    ns.push_back(4'096'000);
    ns.push_back(9'000'000);
    ns.push_back(5'000'000);
    for (int64_t v : ns) s.record(v, 0, 1);
    CHECK(s.lat_over == 3);
    CHECK(s.lat_max_us == 9'000'000 * 1e-3);
    CHECK(s.fine_quantile(0.99) == s.lat_max_us);
    CHECK(s.fine_quantile(0.99) == rule_quantile(ns, 0.99));
    CHECK(s.fine_quantile(0.50) == rule_quantile(ns, 0.50));
  }

  {  // one sample
    LatencyStats s;
    s.record(7'300, 0, 1);
    CHECK(s.fine_quantile(0.50) == 7.375 && s.fine_quantile(0.99) == 7.375);
    ccfd_engine_stats st{};
    s.fill(&st);
    CHECK(st.lat_p50_us == 7.375 && st.lat_p99_us == 7.375 && st.lat_max_us == 7'300 * 1e-3 &&
          st.lat_mean_us == 7'300 * 1e-3);
  }

  {  // nothing completed: fill leaves the four quantile fields alone
    LatencyStats s;
    s.host_wait_ns = 5;
    ccfd_engine_stats st{};
    st.lat_p50_us = -1; st.lat_p99_us = -2; st.lat_max_us = -3; st.lat_mean_us = -4;
    st.host_wait_ns = 99;
    s.fill(&st);
    CHECK(st.lat_p50_us == -1 && st.lat_p99_us == -2 && st.lat_max_us == -3 && st.lat_mean_us == -4);
    CHECK(st.host_wait_ns == 5);
  }

  {  // the two reset scopes
    LatencyStats s;
    fill_everything(s);
    check_state(s, Cleared{false, false});
    s.reset_latency();
    check_state(s, Cleared{true, false});
  }
  {
    LatencyStats s;
    fill_everything(s);
    s.reset_all();
    check_state(s, Cleared{true, true});
    // what fill() writes after a full reset is all zero, and a caller's own fields survive
    ccfd_engine_stats st;
    std::memset(&st, 0xff, sizeof(st));
    const ccfd_engine_stats before = st;
    s.fill(&st);
    CHECK(all_zero(st.lat_hist) && all_zero(st.lat_hist_rows) && all_zero(st.dev_hist) &&
          all_zero(st.dev_hist_rows) && all_zero(st.origin_hist) && all_zero(st.origin_hist_rows));
    CHECK(st.dev_batches == 0 && st.dev_exec_ns == 0 && st.origin_batches == 0);
    CHECK(st.host_submit_ns == 0 && st.host_wait_ns == 0 && st.host_complete_ns == 0);
    CHECK(st.flagged_dropped == before.flagged_dropped && st.flag_full_events == before.flag_full_events);
    CHECK(st.last_seq == before.last_seq && st.last_tx_id == before.last_tx_id &&
          st.last_partition == before.last_partition &&
          std::memcmp(st.last_row, before.last_row, sizeof(st.last_row)) == 0);
    CHECK(st.batches == before.batches && st.rows == before.rows && st.submitted == before.submitted);
  }

  if (g_fail) { std::fprintf(stderr, "lat stats check FAILED (%d)\n", g_fail); return 1; }
  std::printf("lat stats check ok\n");
  return 0;
}

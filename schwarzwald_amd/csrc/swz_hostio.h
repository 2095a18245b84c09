// swz_hostio.h -- what the host-side file writers share (swz_pnts.hip, swz_las.hip): numbers in JSON text and the pool of
// writer threads.
#pragma once

#include <atomic>
#include <charconv>
#include <cmath>
#include <algorithm>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "swz_internal.h"

namespace swz {

inline void put_number(std::string& s, double v) {
  if (v == 0.0 && std::signbit(v)) {  // "-0" is an integer to a parser that tells the two apart, and integers have no sign of zero
    s += "-0.0";
    return;
  }
  char buf[48];
  const auto r = std::to_chars(buf, buf + sizeof(buf), v);  // shortest text that parses back to v
  s.append(buf, r.ptr);
}

// tickets: a few host threads take the items 0 .. num - 1 (the pool swz_bin_persist_nodes uses for its files)
template <typename F>
inline int run_tickets(swz_ctx* c, uint64_t num, F&& item, std::string* first_err) {
  unsigned threads = std::min(32u, std::max(1u, std::thread::hardware_concurrency()));
  if (c) threads = (unsigned)std::max(1L, c->opt_int("SWZ_BIN_WRITER_THREADS", threads));
  threads = (unsigned)std::min<uint64_t>(threads, std::max<uint64_t>(num, 1));
  std::atomic<uint64_t> next{0};
  std::atomic<int> status{SWZ_OK};
  std::mutex err_m;
  auto work = [&]() {
    for (;;) {
      const uint64_t k = next.fetch_add(1);
      if (k >= num || status.load() != SWZ_OK) return;
      std::string err;
      const int st = item(k, &err);
      if (st != SWZ_OK) {
        std::lock_guard<std::mutex> lk(err_m);
        if (status.load() == SWZ_OK) {
          *first_err = err;
          status.store(st);
        }
        return;
      }
    }
  };
  if (threads <= 1) {
    work();
  } else {
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < threads; ++t) pool.emplace_back(work);
    for (auto& t : pool) t.join();
  }
  return status.load();
}

}  // namespace swz

// swz_hostio.h -- what the host side of the node-file writers shares (swz_payload.hip, swz_pnts.hip, swz_las.hip): errors
// with or without a context, whole files in and out, numbers in JSON text and the pool of writer threads.
#pragma once

#include <atomic>
#include <charconv>
#include <cmath>
#include <cstdio>
#include <algorithm>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "swz_internal.h"

namespace swz {

// the entry points of the file writers take a NULL context: then the status is all the caller learns
inline int fail(swz_ctx* c, int code, const std::string& msg) {
  if (c) return c->fail(code, msg.c_str());
  return code;
}

inline bool finite3(const double v[3]) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

inline int read_whole_file(swz_ctx* c, const char* path, std::vector<unsigned char>* out) {
  FILE* f = fopen(path, "rb");
  if (!f) return fail(c, SWZ_ERR_BAD_ARG, std::string("cannot open ") + path);
  unsigned char tmp[1 << 16];
  size_t got;
  while ((got = fread(tmp, 1, sizeof(tmp), f)) > 0) out->insert(out->end(), tmp, tmp + got);
  fclose(f);
  return SWZ_OK;
}

// A file out of pieces that go out as they lie in memory, one behind the other.  No context: the files of a table are
// written by several threads (run_tickets).
struct FilePiece {
  const void* data;
  size_t bytes;
};
inline int write_file(const std::string& path, const std::vector<FilePiece>& pieces, std::string* err) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) {
    *err = "cannot write " + path;
    return SWZ_ERR_BAD_ARG;
  }
  bool ok = true;
  for (const FilePiece& p : pieces) ok = ok && fwrite(p.data, 1, p.bytes, f) == p.bytes;
  ok = (fclose(f) == 0) && ok;
  if (!ok) {
    *err = "short write to " + path;
    return SWZ_ERR_INTERNAL;
  }
  return SWZ_OK;
}

inline void put_number(std::string& s, double v) {
  if (v == 0.0 && std::signbit(v)) {  // "-0" is an integer to a parser that tells the two apart, and integers have no sign of zero
    s += "-0.0";
    return;
  }
  char buf[48];
  const auto r = std::to_chars(buf, buf + sizeof(buf), v);  // shortest text that parses back to v
  s.append(buf, r.ptr);
}

// tickets: a few host threads take the items 0 .. num - 1, which are independent -- the files of a node table (the
// reference persists its nodes from the tasks of its tiling graph, TilingAlgorithms.cpp:330-334).  One thread wrote
// 2.7 GB/s of BIN files -- a hundredth of what the device hands over.  SWZ_BIN_WRITER_THREADS: the number of threads
// (default: the host's, at most 32).  The first item that fails ends the run; its status and text come back.
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

// swz_hostio.h -- what the host side of the node-file writers shares (swz_payload.hip, swz_binpack.hip, swz_pnts.hip,
// swz_las.hip, swz_toutput.hip) and the readers of a written data set: errors with or without a context (why_text: into a
// caller's text buffer), host wall time (ms_since), whole files in and out, numbers in JSON text, the pool of writer threads
// and the attribute arrays of a BIN node file.
#pragma once

#include <fcntl.h>
#include <unistd.h>
#include <zlib.h>

#include <atomic>
#include <chrono>
#include <charconv>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstring>
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

static const uint32_t ATTR_BYTES[SWZ_ATTR_COUNT] = {3, 12, 2, 1, 1, 8, 1, 1, 2, 1, 1, 1};
// order of the attribute arrays in a node file (BinaryPersistence.h:120-190: bit 10 before bit 9)
static const int FILE_ORDER[SWZ_ATTR_COUNT] = {SWZ_ATTR_RGB, SWZ_ATTR_NORMAL, SWZ_ATTR_INTENSITY, SWZ_ATTR_CLASSIFICATION,
                                               SWZ_ATTR_EDGE_OF_FLIGHT_LINE, SWZ_ATTR_GPS_TIME, SWZ_ATTR_NUMBER_OF_RETURNS,
                                               SWZ_ATTR_RETURN_NUMBER, SWZ_ATTR_POINT_SOURCE_ID, SWZ_ATTR_SCAN_ANGLE_RANK,
                                               SWZ_ATTR_SCAN_DIRECTION_FLAG, SWZ_ATTR_USER_DATA};

inline bool finite3(const double v[3]) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// host wall time since t0, for the *_ms fields of the calls' stats
inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// the end of a host-only entry that reports through a text buffer: the refusal that `text` holds (nothing on SWZ_OK) goes
// into why_out, cut to why_bytes with its terminator; returns st
inline int why_text(int st, const swz_ctx& text, char* why_out, uint64_t why_bytes) {
  if (why_out && why_bytes) {
    const size_t len = std::min<size_t>(st == SWZ_OK ? 0 : text.err.size(), (size_t)why_bytes - 1);
    memcpy(why_out, text.err.data(), len);
    why_out[len] = 0;
  }
  return st;
}

inline int read_whole_file(swz_ctx* c, const char* path, std::vector<unsigned char>* out) {
  FILE* f = fopen(path, "rb");
  if (!f) return fail(c, SWZ_ERR_BAD_ARG, std::string("cannot open ") + path);
  unsigned char tmp[1 << 16];
  size_t got;
  while ((got = fread(tmp, 1, sizeof(tmp), f)) > 0) out->insert(out->end(), tmp, tmp + got);
  fclose(f);
  return SWZ_OK;
}

// `bytes` bytes at `offset` of the file, all of them or an error
inline bool pread_all(int fd, void* dst, uint64_t bytes, uint64_t offset) {
  unsigned char* out = static_cast<unsigned char*>(dst);
  while (bytes) {
    const ssize_t got = pread(fd, out, (size_t)std::min<uint64_t>(bytes, 1ull << 30), (off_t)offset);
    if (got < 0 && errno == EINTR) continue;
    if (got <= 0) return false;
    out += got;
    offset += (uint64_t)got;
    bytes -= (uint64_t)got;
  }
  return true;
}

struct Fd {
  int fd = -1;
  ~Fd() {
    if (fd >= 0) (void)close(fd);
  }
};

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

// the same bytes as ONE zlib stream, level 1 (BinaryPersistence's .binz).  A stream zlib could not make leaves an empty file
// and is reported like a write that failed.
inline int write_file_zlib(const std::string& path, const void* data, size_t bytes, std::string* err) {
  uLongf cap = compressBound((uLong)bytes);
  std::vector<unsigned char> z(cap);
  const bool packed = compress2(z.data(), &cap, static_cast<const Bytef*>(data), (uLong)bytes, Z_BEST_SPEED) == Z_OK;
  const int st = write_file(path, {{z.data(), packed ? (size_t)cap : 0}}, err);
  if (st != SWZ_OK || packed) return st;
  *err = "short write to " + path;
  return SWZ_ERR_INTERNAL;
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

// The same pool, started and joined in two steps: the caller goes on (packs and copies the next chunk of a tiler's output,
// swz_toutput.hip) while the items are worked off.  As many threads as run_tickets would take, never the caller's own.
class TicketRun {
public:
  TicketRun() = default;
  TicketRun(const TicketRun&) = delete;
  TicketRun& operator=(const TicketRun&) = delete;
  ~TicketRun() { (void)wait(nullptr, nullptr); }

  // want_threads > 0: that many threads (a caller with an option of its own: the readers of swz_tinput.hip; or with a share
  // of the option's budget: the shards of swz_group_write_output)
  template <typename F>
  void start(swz_ctx* c, uint64_t num, F item, long want_threads = 0) {
    unsigned threads = std::min(32u, std::max(1u, std::thread::hardware_concurrency()));
    if (want_threads > 0) threads = (unsigned)want_threads;
    else if (c) threads = (unsigned)std::max(1L, c->opt_int("SWZ_BIN_WRITER_THREADS", threads));
    threads = (unsigned)std::min<uint64_t>(threads, std::max<uint64_t>(num, 1));
    next_.store(0);
    status_.store(SWZ_OK);
    err_.clear();
    begin_ = std::chrono::steady_clock::now();
    busy_ms_ = 0.0;
    for (unsigned t = 0; t < threads; ++t)
      pool_.emplace_back([this, num, item]() {
        for (;;) {
          const uint64_t k = next_.fetch_add(1);
          if (k >= num || status_.load() != SWZ_OK) break;
          std::string err;
          const int st = item(k, &err);
          if (st != SWZ_OK) {
            std::lock_guard<std::mutex> lk(m_);
            if (status_.load() == SWZ_OK) {
              err_ = err;
              status_.store(st);
            }
            break;
          }
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - begin_).count();
        std::lock_guard<std::mutex> lk(m_);
        busy_ms_ = std::max(busy_ms_, ms);
      });
  }
  bool running() const { return !pool_.empty(); }
  // joins; the status of the first item that failed and its text; *busy_ms: from start() to the last thread's end
  int wait(std::string* first_err, double* busy_ms) {
    for (auto& t : pool_) t.join();
    const bool ran = !pool_.empty();
    pool_.clear();
    if (first_err && status_.load() != SWZ_OK) *first_err = err_;
    if (busy_ms) *busy_ms = ran ? busy_ms_ : 0.0;
    return status_.load();
  }

private:
  std::vector<std::thread> pool_;
  std::atomic<uint64_t> next_{0};
  std::atomic<int> status_{SWZ_OK};
  std::mutex m_;
  std::string err_;
  std::chrono::steady_clock::time_point begin_;
  double busy_ms_ = 0.0;
};

}  // namespace swz

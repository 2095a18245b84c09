// Shared by test_adapter_seams.cpp and test_adapter_tiler.cpp: a seeded generator, the clouds of the Python
// tests written again in C++, bit comparison of doubles and the failure plumbing (a failed CHECK ends the
// executable with one "FAIL:" line).  Test code only.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace seam {

struct Failure : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define SEAM_STR2(x) #x
#define SEAM_STR(x) SEAM_STR2(x)
#define CHECK(cond, ...)                                                                              \
  do {                                                                                                \
    if (!(cond)) {                                                                                    \
      char seam_buf[512];                                                                             \
      std::snprintf(seam_buf, sizeof seam_buf, "" __VA_ARGS__);                                       \
      throw seam::Failure{std::string(#cond " (" __FILE__ ":" SEAM_STR(__LINE__) ") ") + seam_buf};   \
    }                                                                                                 \
  } while (0)

inline uint64_t bits(double v) {
  uint64_t u;
  std::memcpy(&u, &v, 8);
  return u;
}

struct Rng {  // splitmix64
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed) {}
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double uniform() { return (double)(next() >> 11) * 0x1.0p-53; }
  uint64_t below(uint64_t n) { return next() % n; }
  double normal() {  // Box-Muller
    const double u = 1.0 - uniform(), v = uniform();
    return std::sqrt(-2.0 * std::log(u)) * std::cos(6.283185307179586 * v);
  }
};

struct Box {
  double mn[3], mx[3];
  double ext(int a) const { return mx[a] - mn[a]; }
};
// the bounds of tests/test_multibatch.py: off the origin, not a power of two wide
inline Box odd_box() {
  Box b{{-512.25, 1000.5, -3.125}, {0, 0, 0}};
  for (int a = 0; a < 3; ++a) b.mx[a] = b.mn[a] + 777.7;
  return b;
}
inline Box unit_box() { return Box{{0, 0, 0}, {1, 1, 1}}; }
inline Box cube_box(double side) { return Box{{0, 0, 0}, {side, side, side}}; }

inline double clamp01(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }

inline void shuffle_points(Rng& r, std::vector<double>& u) {
  const size_t n = u.size() / 3;
  for (size_t i = n; i > 1; --i) {
    const size_t j = (size_t)r.below(i);
    for (int a = 0; a < 3; ++a) std::swap(u[3 * (i - 1) + a], u[3 * j + a]);
  }
}
inline std::vector<double> scale_into(const std::vector<double>& u, const Box& b) {
  std::vector<double> out(u.size());
  for (size_t i = 0; i < u.size(); ++i) out[i] = b.mn[i % 3] + u[i] * b.ext((int)(i % 3));
  return out;
}

inline std::vector<double> uniform_cloud(Rng& r, size_t n, const Box& b) {
  std::vector<double> u(3 * n);
  for (double& v : u) v = r.uniform();
  return scale_into(u, b);
}

// tests/test_gpu_parity.py:_clustered -- two thin planes, a blob and exact duplicates of a few base points
inline std::vector<double> clustered_surfaces(Rng& r, size_t n, const Box& b) {
  std::vector<double> u;
  u.reserve(3 * n);
  const size_t k = n / 4;
  for (size_t i = 0; i < k; ++i) { u.push_back(r.uniform()); u.push_back(r.uniform()); u.push_back(0.3 + 0.001 * r.normal()); }
  for (size_t i = 0; i < k; ++i) { u.push_back(r.uniform()); u.push_back(0.7 + 0.0005 * r.normal()); u.push_back(r.uniform()); }
  for (size_t i = 0; i < 3 * k; ++i) u.push_back(0.5 + 0.02 * r.normal());
  const size_t rest = n - 3 * k, nb = std::max<size_t>(rest / 8, 1);
  std::vector<double> base(3 * nb);
  for (double& v : base) v = r.uniform();
  for (size_t i = 0; i < rest; ++i) {
    const size_t j = (size_t)r.below(nb);
    for (int a = 0; a < 3; ++a) u.push_back(base[3 * j + a]);
  }
  for (double& v : u) v = clamp01(v);
  shuffle_points(r, u);
  return scale_into(u, b);
}

// tests/test_multibatch.py:_points(clustered=True) -- a plane, a blob and exact duplicates, shuffled so that equal
// points (equal keys) land in different batches
inline std::vector<double> clustered_duplicates(Rng& r, size_t n, const Box& b) {
  std::vector<double> u;
  u.reserve(3 * n);
  const size_t k = n / 3;
  for (size_t i = 0; i < k; ++i) { u.push_back(r.uniform()); u.push_back(r.uniform()); u.push_back(0.3 + 0.002 * r.normal()); }
  for (size_t i = 0; i < 3 * k; ++i) u.push_back(0.6 + 0.03 * r.normal());
  const size_t rest = n - 2 * k, nb = std::max<size_t>(rest / 6, 1);
  std::vector<double> base(3 * nb);
  for (double& v : base) v = r.uniform();
  for (size_t i = 0; i < rest; ++i) {
    const size_t j = (size_t)r.below(nb);
    for (int a = 0; a < 3; ++a) u.push_back(base[3 * j + a]);
  }
  for (double& v : u) v = clamp01(v);
  shuffle_points(r, u);
  return scale_into(u, b);
}

// "r" + octant digits (core/tiling/TilingAlgorithms.cpp:139), written without the library or the adapter
inline std::string node_name(int level, uint64_t key) {
  std::string s = "r";
  for (int l = 0; l <= level; ++l) s.push_back((char)('0' + ((key >> ((20 - l) * 3)) & 7u)));
  return s;
}

inline float spacing_from_diagonal(const Box& b, double divisor) {
  const double dx = b.ext(0), dy = b.ext(1), dz = b.ext(2);
  return (float)(std::sqrt(dx * dx + dy * dy + dz * dz) / divisor);
}

}  // namespace seam

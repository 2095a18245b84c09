// The sampling-strategy factories of the host adapter and MIN_DISTANCE_FAST: make_sampling_strategy (the five names of
// TilerProcess::make_sampling_strategy, TilerProcess.cpp:491-516) builds the adaptive sampler with the command line's
// densities; make_sampling_strategy_from_name (Sampling.h:774-791) has no densities to build it with and throws.
// Pure host code: no swz_host::Context is created.
#include <cstdio>
#include <stdexcept>
#include <string>

#include "../../schwarzwald_amd/host/swz_tiling.hpp"

static int failures = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      std::printf("FAILED %s: ", #cond);      \
      std::printf(__VA_ARGS__);               \
      std::printf("\n");                      \
      ++failures;                             \
    }                                         \
  } while (0)

int main() {
  using namespace swz_host;
  const SamplingStrategy fast = make_sampling_strategy("MIN_DISTANCE_FAST", 7);
  CHECK(fast.kind == SWZ_MIN_DISTANCE_FAST && fast.kind == 4, "kind %d", fast.kind);
  CHECK(fast.max_points_per_node == 7, "max_points_per_node %zu", fast.max_points_per_node);
  CHECK(fast.density_per_level != nullptr, "no densities attached");
  if (fast.density_per_level) {
    const int32_t levels[] = {-1, 0, 1, 2, 20};
    const float expect[] = {0.25f, 0.5f, 1.f, 1.f, 1.f};
    for (int k = 0; k < 5; ++k)
      CHECK(fast.density_per_level(levels[k]) == expect[k], "density(%d) = %g", levels[k], (double)fast.density_per_level(levels[k]));
  }
  std::printf("factory five names ok: MIN_DISTANCE_FAST -> kind %d\n", fast.kind);

  const char* names[] = {"RANDOM_GRID", "GRID_CENTER", "MIN_DISTANCE", "JITTERED"};
  for (int s = 0; s < 4; ++s) {
    const SamplingStrategy a = make_sampling_strategy(names[s], 123), b = make_sampling_strategy_from_name(names[s], 123);
    CHECK(a.kind == s && b.kind == s && a.max_points_per_node == 123 && a.density_per_level == nullptr, "%s", names[s]);
  }
  std::printf("factory four names ok: both factories agree\n");

  bool threw = false;
  try {
    (void)make_sampling_strategy_from_name("MIN_DISTANCE_FAST", 7);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw, "make_sampling_strategy_from_name(\"MIN_DISTANCE_FAST\") did not throw");
  for (const char* bad : {"", "min_distance_fast", "POISSON"}) {
    bool t2 = false;
    try {
      (void)make_sampling_strategy(bad, 7);
    } catch (const std::invalid_argument&) {
      t2 = true;
    }
    CHECK(t2, "make_sampling_strategy(\"%s\") did not throw", bad);
  }
  std::printf("factory refusals ok: from_name still throws for MIN_DISTANCE_FAST\n");
  return failures ? 1 : 0;
}

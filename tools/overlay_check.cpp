// Host check of dr::overlay_lower_bound / dr::overlay_find
// (deeprec-1_amd/csrc/dr_overlay.h) against std::lower_bound over random
// sorted int64 ranges: empty ranges, one key, the keys -1, 0, INT64_MIN and
// INT64_MAX, sub-ranges [lo, hi) of a longer array (a table's range of a
// grouped overlay), and probes below, above, between and on the keys.
//
//   g++ -O2 -std=c++17 -I deeprec-1_amd/csrc tools/overlay_check.cpp -o overlay_check
//   ./overlay_check <cases> <seed>      ->  "... mismatches 0", exit 0
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "dr_overlay.h"

static const int64_t kMin = std::numeric_limits<int64_t>::min();
static const int64_t kMax = std::numeric_limits<int64_t>::max();

static long long g_checks = 0, g_bad = 0;

static void check_one(const std::vector<int64_t>& keys, int64_t lo, int64_t hi, int64_t probe) {
  const int64_t* b = keys.data();
  const int64_t want = lo >= hi ? lo : std::lower_bound(b + lo, b + hi, probe) - b;
  const int64_t got = dr::overlay_lower_bound(b, lo, hi, probe);
  const bool member = lo < hi && std::binary_search(b + lo, b + hi, probe);
  const int64_t f = dr::overlay_find(b, lo, hi, probe);
  const bool ok = got == want && (member ? (f == want && b[f] == probe) : f == -1);
  ++g_checks;
  if (!ok) {
    if (++g_bad <= 10)
      printf("MISMATCH n=%zu lo=%lld hi=%lld probe=%lld: lower_bound %lld (want %lld), find %lld\n",
             keys.size(), (long long)lo, (long long)hi, (long long)probe, (long long)got,
             (long long)want, (long long)f);
  }
}

// Every probe worth asking of keys[lo, hi): each key, its neighbours, the
// midpoints between adjacent keys, the extremes, and a few random values.
static void check_range(const std::vector<int64_t>& keys, int64_t lo, int64_t hi,
                        std::mt19937_64& rng) {
  std::vector<int64_t> probes = {kMin, kMin + 1, -2, -1, 0, 1, kMax - 1, kMax};
  for (int64_t i = lo; i < hi; ++i) {
    const int64_t k = keys[i];
    probes.push_back(k);
    if (k > kMin) probes.push_back(k - 1);
    if (k < kMax) probes.push_back(k + 1);
    if (i + 1 < hi) {
      // midpoint without overflow
      const int64_t a = k, c = keys[i + 1];
      probes.push_back(a / 2 + c / 2);
    }
  }
  for (int r = 0; r < 8; ++r) probes.push_back((int64_t)rng());
  for (int64_t p : probes) check_one(keys, lo, hi, p);
}

static std::vector<int64_t> sorted_unique(std::vector<int64_t> v) {
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  return v;
}

int main(int argc, char** argv) {
  const long long cases = argc > 1 ? atoll(argv[1]) : 2000;
  const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
  std::mt19937_64 rng(seed);

  // fixed cases first: empty, M = 1, the special keys
  check_range({}, 0, 0, rng);
  check_range({5}, 0, 0, rng);      // an empty range of a non-empty array
  check_range({5}, 1, 1, rng);
  for (int64_t k : {(int64_t)-1, (int64_t)0, kMin, kMax, (int64_t)42}) check_range({k}, 0, 1, rng);
  check_range({kMin, -1, 0, kMax}, 0, 4, rng);
  check_range({kMin, -1, 0, kMax}, 1, 3, rng);
  check_range({kMin, kMin + 1, kMax - 1, kMax}, 0, 4, rng);

  for (long long c = 0; c < cases; ++c) {
    const int shape = (int)(rng() % 4);
    const size_t n = shape == 0 ? rng() % 4 : (shape == 1 ? rng() % 40 : rng() % 1200);
    std::vector<int64_t> v;
    for (size_t i = 0; i < n; ++i) {
      switch (rng() % 4) {
        case 0: v.push_back((int64_t)rng()); break;                       // anywhere
        case 1: v.push_back((int64_t)(rng() % 64) - 32); break;           // dense around zero
        case 2: v.push_back(kMin + (int64_t)(rng() % 16)); break;         // at the bottom
        default: v.push_back(kMax - (int64_t)(rng() % 16)); break;        // at the top
      }
    }
    if (rng() % 3 == 0) {
      const int64_t sp[4] = {-1, 0, kMin, kMax};
      for (int64_t k : sp)
        if (rng() % 2) v.push_back(k);
    }
    // a grouped overlay: T ranges, each sorted on its own, laid back to back
    const int T = 1 + (int)(rng() % 3);
    std::vector<int64_t> all;
    std::vector<int64_t> off = {0};
    for (int t = 0; t < T; ++t) {
      std::vector<int64_t> part;
      for (int64_t k : v)
        if (T == 1 || rng() % T == (uint64_t)t || rng() % 4 == 0) part.push_back(k);
      if (rng() % 5 == 0) part.clear();   // an empty range in the middle
      part = sorted_unique(part);
      all.insert(all.end(), part.begin(), part.end());
      off.push_back((int64_t)all.size());
    }
    for (int t = 0; t < T; ++t) check_range(all, off[t], off[t + 1], rng);
  }
  printf("checks %lld mismatches %lld\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}

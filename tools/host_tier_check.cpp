// host_tier_check.cpp -- dr::HostTier (deeprec-1_amd/csrc/dr_host_tier.h)
// walked against std::map: seeded random put / take (erase 0 and 1) / remove /
// shrink, the full export compared with the model after every operation.
// Starts at capacity_hint 1 so the map rehashes several times; the key pool
// holds -1, 0, INT64_MIN, INT64_MAX and keys that share one home bucket of the
// largest map the walk reaches.  Built with -fsanitize=address,undefined by
// tests/test_host_tier_sanitized.py.
//
//   host_tier_check <operations> <seed>     prints "mismatches <n>"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <random>
#include <set>
#include <vector>

#include "dr_host_tier.h"

namespace {

constexpr int kCols = 3;
const int64_t kColBytes[kCols] = {4, 32, 10};

struct Entry {
  int64_t version, freq;
  uint32_t colmask;
  std::vector<uint8_t> v[kCols];
  bool operator==(const Entry& o) const {
    if (version != o.version || freq != o.freq || colmask != o.colmask) return false;
    for (int c = 0; c < kCols; ++c)
      if (v[c] != o.v[c]) return false;
    return true;
  }
};

uint64_t mix64(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdULL;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ULL;
  k ^= k >> 33;
  return k;
}

struct Columns {  // n rows per column, and the pointer array the tier takes
  std::vector<uint8_t> buf[kCols];
  void* p[kCols];
  explicit Columns(int64_t n) {
    for (int c = 0; c < kCols; ++c) {
      buf[c].assign((size_t)(n * kColBytes[c]) + 1, 0xA5);
      p[c] = buf[c].data();
    }
  }
  std::vector<uint8_t> row(int c, int64_t j) const {
    return std::vector<uint8_t>(buf[c].begin() + j * kColBytes[c],
                                buf[c].begin() + (j + 1) * kColBytes[c]);
  }
};

int64_t check_export(dr::HostTier& t, const std::map<int64_t, Entry>& model) {
  const int64_t m = t.size();
  if (m != (int64_t)model.size()) return 1;
  std::vector<int64_t> keys((size_t)m + 1), ver((size_t)m + 1), frq((size_t)m + 1);
  std::vector<uint32_t> cm((size_t)m + 1);
  Columns cols(m);
  t.export_all(keys.data(), cols.p, ver.data(), frq.data(), cm.data());
  int64_t bad = 0, j = 0;
  for (const auto& kv : model) {  // std::map iterates ascending as signed int64
    Entry e{ver[(size_t)j], frq[(size_t)j], cm[(size_t)j], {}};
    for (int c = 0; c < kCols; ++c) e.v[c] = cols.row(c, j);
    if (keys[(size_t)j] != kv.first || !(e == kv.second)) ++bad;
    ++j;
  }
  return bad;
}

}  // namespace

int main(int argc, char** argv) {
  const int64_t ops = argc > 1 ? atoll(argv[1]) : 2000;
  const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
  std::mt19937_64 rng(seed);
  std::vector<int64_t> pool = {-1, 0, INT64_MIN, INT64_MAX, 1, -2};
  for (uint64_t k = 1; pool.size() < 300; ++k)  // one home bucket of a 4096-bucket map
    if ((mix64(k * 0x9E3779B97F4A7C15ULL) & 4095) == 77) pool.push_back((int64_t)(k * 0x9E3779B97F4A7C15ULL));
  while (pool.size() < 900) pool.push_back((int64_t)rng());
  auto draw = [&](int64_t n) {
    std::vector<int64_t> k((size_t)n);
    for (auto& x : k) x = pool[rng() % pool.size()];
    return k;
  };

  dr::HostTier t(kCols, kColBytes, 1);
  std::map<int64_t, Entry> model;
  int64_t bad = 0, max_buckets = t.buckets(), gs = 0;
  for (int64_t op = 0; op < ops; ++op) {
    const int kind = (int)(rng() % 10);
    const int64_t n = (int64_t)(rng() % 40);
    const std::vector<int64_t> keys = draw(n);
    if (kind < 4) {  // put: the last occurrence of a repeated key wins
      Columns cols(n);
      std::vector<int64_t> ver((size_t)n + 1), frq((size_t)n + 1);
      std::vector<uint32_t> cm((size_t)n + 1);
      for (int64_t i = 0; i < n; ++i) {
        ver[(size_t)i] = rng() % 5 == 0 ? -1 : (int64_t)(rng() % 64);
        frq[(size_t)i] = (int64_t)(rng() % 9);
        cm[(size_t)i] = (uint32_t)(rng() % 8);
        for (int c = 0; c < kCols; ++c)
          for (int64_t b = 0; b < kColBytes[c]; ++b)
            cols.buf[c][(size_t)(i * kColBytes[c] + b)] = (uint8_t)rng();
      }
      t.put(keys.data(), n, cols.p, ver.data(), frq.data(), cm.data());
      for (int64_t i = 0; i < n; ++i) {
        Entry e{ver[(size_t)i], frq[(size_t)i], cm[(size_t)i], {}};
        for (int c = 0; c < kCols; ++c) e.v[c] = cols.row(c, i);
        model[keys[(size_t)i]] = e;
      }
    } else if (kind < 7) {  // take, erase 0 / 1
      const int erase = (int)(rng() & 1);
      Columns cols(n);
      std::vector<int64_t> idx((size_t)n + 1), ver((size_t)n + 1), frq((size_t)n + 1);
      std::vector<uint32_t> cm((size_t)n + 1);
      const int64_t hits = t.take(keys.data(), n, erase, idx.data(), cols.p, ver.data(), frq.data(),
                                  cm.data());
      std::set<int64_t> seen;
      int64_t j = 0;
      for (int64_t i = 0; i < n; ++i) {
        auto it = model.find(keys[(size_t)i]);
        if (it == model.end() || !seen.insert(keys[(size_t)i]).second) continue;
        if (j < hits) {
          Entry e{ver[(size_t)j], frq[(size_t)j], cm[(size_t)j], {}};
          for (int c = 0; c < kCols; ++c) e.v[c] = cols.row(c, j);
          if (idx[(size_t)j] != i || !(e == it->second)) ++bad;
        }
        ++j;
      }
      if (j != hits) ++bad;
      if (erase)
        for (int64_t k : seen) model.erase(k);
    } else if (kind < 9) {  // remove
      std::set<int64_t> gone;
      for (int64_t k : keys)
        if (model.erase(k)) gone.insert(k);
      if (t.remove(keys.data(), n) != (int64_t)gone.size()) ++bad;
    } else {  // shrink
      gs += (int64_t)(rng() % 8);
      const int64_t stl = (int64_t)(rng() % 48);
      int64_t dropped = 0;
      for (auto it = model.begin(); it != model.end();) {
        if (it->second.version == -1) {
          it->second.version = gs;
          ++it;
        } else if (gs - it->second.version > stl) {
          it = model.erase(it);
          ++dropped;
        } else {
          ++it;
        }
      }
      if (t.shrink(gs, stl) != dropped) ++bad;
    }
    bad += check_export(t, model);
    if (t.buckets() > max_buckets) max_buckets = t.buckets();
  }
  printf("operations %lld final %lld buckets %lld mismatches %lld\n", (long long)ops,
         (long long)t.size(), (long long)max_buckets, (long long)bad);
  return bad ? 1 : 0;
}

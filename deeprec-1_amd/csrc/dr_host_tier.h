// dr_host_tier.h -- the host-DRAM tier of an HBM_DRAM EmbeddingVariable
// (DESIGN section 16): the keys the HBM budget demoted, with everything a
// promotion needs to put them back exactly -- version, freq, the first-touch
// bits of the key space's columns (colmask) and one value row per column.
//
// Layout:
//   map      open addressing, linear probing from mix64(key) & mask, int64
//            ENTRY INDEX per bucket (-1 = empty: the marker is not a key value,
//            so -1, 0, INT64_MIN and INT64_MAX are ordinary keys).  Deletion
//            shifts the run back (no tombstones); the map doubles by rehash
//            once it is 3/4 full.
//   entries  parallel arrays key / version / freq / colmask and one value slab
//            per column (col_bytes[c] bytes per entry); a freed entry goes on
//            the free list and is handed out again before the arrays grow.
// Plain host memory, single-threaded: the caller holds the primary EV's lock.
//
// Header-only and host-compilable (tools/host_tier_check.cpp and
// tools/host_tier_flags_check.cpp walk it against std::map under the
// sanitizers; the C entries are in host_tier.hip).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace dr {

class HostTier {
 public:
  HostTier(int ncols, const int64_t* col_bytes, int64_t capacity_hint)
      : col_bytes_(col_bytes, col_bytes + ncols), slabs_((size_t)ncols) {
    int64_t cap = 8;
    while (cap * 3 < std::max<int64_t>(capacity_hint, 0) * 4) cap *= 2;
    map_.assign((size_t)cap, -1);
  }

  int ncols() const { return (int)col_bytes_.size(); }
  int64_t col_bytes(int c) const { return col_bytes_[(size_t)c]; }
  int64_t size() const { return size_; }
  int64_t buckets() const { return (int64_t)map_.size(); }

  // values[c] (nullable, as `values` itself): n rows of col_bytes[c]; a null
  // column leaves the entry's row as it is (zeros for a new entry).  versions
  // / freqs / colmask nullable: 0.  An existing key is overwritten.
  void put(const int64_t* keys, int64_t n, const void* const* values, const int64_t* versions,
           const int64_t* freqs, const uint32_t* colmask) {
    for (int64_t i = 0; i < n; ++i) {
      int64_t e = find(keys[i]);
      if (e < 0) e = insert_new(keys[i]);
      version_[(size_t)e] = versions ? versions[i] : 0;
      freq_[(size_t)e] = freqs ? freqs[i] : 0;
      colmask_[(size_t)e] = colmask ? colmask[i] : 0u;
      for (int c = 0; c < ncols(); ++c) {
        const int64_t b = col_bytes_[(size_t)c];
        if (values && values[c] && b)
          memcpy(&slabs_[(size_t)c][(size_t)(e * b)],
                 static_cast<const char*>(values[c]) + i * b, (size_t)b);
      }
    }
  }

  // Hits compacted in input order: hit j is input position hit_index_out[j].
  // A key repeated in the input hits once, at its first position.  Every
  // output is nullable.  erase: the hits leave the tier.  Returns the hits.
  int64_t take(const int64_t* keys, int64_t n, int erase, int64_t* hit_index_out,
               void* const* values_out, int64_t* versions_out, int64_t* freqs_out,
               uint32_t* colmask_out) {
    hit_.clear();
    int64_t h = 0;
    for (int64_t i = 0; i < n; ++i) {
      const int64_t e = find(keys[i]);
      if (e < 0 || seen_[(size_t)e]) continue;
      seen_[(size_t)e] = 1;
      hit_.push_back(e);
      if (hit_index_out) hit_index_out[h] = i;
      copy_out(e, h, values_out, versions_out, freqs_out, colmask_out);
      ++h;
    }
    for (int64_t e : hit_) {
      seen_[(size_t)e] = 0;
      if (erase) erase_entry(e);
    }
    return h;
  }

  // Absent keys are ignored, duplicates count once.  Returns the keys removed.
  int64_t remove(const int64_t* keys, int64_t n) {
    int64_t r = 0;
    for (int64_t i = 0; i < n; ++i) {
      const int64_t e = find(keys[i]);
      if (e >= 0) {
        erase_entry(e);
        ++r;
      }
    }
    return r;
  }

  // The age rule of ev_shrink_mark_kernel's mode 2 (EmbeddingVar::Shrink,
  // embedding_var.h:264-313): version == -1 -> version = global_step, kept;
  // global_step - version > steps_to_live -> dropped.  Returns the keys dropped.
  int64_t shrink(int64_t global_step, int64_t steps_to_live) {
    hit_.clear();
    for (int64_t e : map_) {
      if (e < 0) continue;
      int64_t& ver = version_[(size_t)e];
      if (ver == -1)
        ver = global_step;
      else if (global_step - ver > steps_to_live)
        hit_.push_back(e);
    }
    for (int64_t e : hit_) erase_entry(e);
    return (int64_t)hit_.size();
  }

  // shrink() with the dropped keys written to keys_out (any order; the caller
  // sizes it for size() entries).
  int64_t shrink_keys(int64_t global_step, int64_t steps_to_live, int64_t* keys_out) {
    hit_.clear();
    for (int64_t e : map_) {
      if (e < 0) continue;
      int64_t& ver = version_[(size_t)e];
      if (ver == -1)
        ver = global_step;
      else if (global_step - ver > steps_to_live)
        hit_.push_back(e);
    }
    for (size_t j = 0; j < hit_.size(); ++j) {
      keys_out[j] = key_[(size_t)hit_[j]];
      erase_entry(hit_[j]);
    }
    return (int64_t)hit_.size();
  }

  // -- colmask as a flag word: bits 0-15 are the first-
  // touch bits, bit 16 is "updated since the last delta" (DR_TIER_UPDATED); the
  // store treats every bit alike.
  // Entries with (colmask & mask) == mask.
  int64_t count_masked(uint32_t mask) const {
    int64_t n = 0;
    for (int64_t e : map_)
      if (e >= 0 && (colmask_[(size_t)e] & mask) == mask) ++n;
    return n;
  }

  // export_all narrowed to the entries count_masked(mask) counts; the caller
  // sizes the outputs for that many.  Returns the entries written.
  int64_t export_masked(uint32_t mask, int64_t* keys_out, void* const* values_out,
                        int64_t* versions_out, int64_t* freqs_out, uint32_t* colmask_out) {
    hit_.clear();
    for (int64_t e : map_)
      if (e >= 0 && (colmask_[(size_t)e] & mask) == mask) hit_.push_back(e);
    std::sort(hit_.begin(), hit_.end(),
              [this](int64_t a, int64_t b) { return key_[(size_t)a] < key_[(size_t)b]; });
    for (size_t j = 0; j < hit_.size(); ++j) {
      if (keys_out) keys_out[j] = key_[(size_t)hit_[j]];
      copy_out(hit_[j], (int64_t)j, values_out, versions_out, freqs_out, colmask_out);
    }
    return (int64_t)hit_.size();
  }

  // colmask &= ~mask on every entry.  Returns the entries that changed.
  int64_t clear_bits(uint32_t mask) {
    int64_t n = 0;
    for (int64_t e : map_) {
      if (e < 0 || !(colmask_[(size_t)e] & mask)) continue;
      colmask_[(size_t)e] &= ~mask;
      ++n;
    }
    return n;
  }

  // colmask |= bits on each distinct key present with (colmask & require) ==
  // require; absent keys are ignored.  Returns the distinct keys that met the
  // requirement (whether or not their word changed).
  int64_t or_bits(const int64_t* keys, int64_t n, uint32_t require, uint32_t bits) {
    hit_.clear();
    for (int64_t i = 0; i < n; ++i) {
      const int64_t e = find(keys[i]);
      if (e < 0 || seen_[(size_t)e]) continue;
      seen_[(size_t)e] = 1;
      hit_.push_back(e);
    }
    int64_t h = 0;
    for (int64_t e : hit_) {
      seen_[(size_t)e] = 0;
      if ((colmask_[(size_t)e] & require) != require) continue;
      colmask_[(size_t)e] |= bits;
      ++h;
    }
    return h;
  }

  // Every entry, keys ascending as signed int64; outputs nullable, sized for
  // size() entries by the caller.
  void export_all(int64_t* keys_out, void* const* values_out, int64_t* versions_out,
                  int64_t* freqs_out, uint32_t* colmask_out) {
    hit_.clear();
    for (int64_t e : map_)
      if (e >= 0) hit_.push_back(e);
    std::sort(hit_.begin(), hit_.end(),
              [this](int64_t a, int64_t b) { return key_[(size_t)a] < key_[(size_t)b]; });
    for (size_t j = 0; j < hit_.size(); ++j) {
      if (keys_out) keys_out[j] = key_[(size_t)hit_[j]];
      copy_out(hit_[j], (int64_t)j, values_out, versions_out, freqs_out, colmask_out);
    }
  }

 private:
  static uint64_t mix64(uint64_t k) {  // dr_common.h's, restated for the host
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return k;
  }
  size_t home(int64_t key) const { return (size_t)(mix64((uint64_t)key) & (map_.size() - 1)); }

  // bucket of `key`, or of the empty bucket that ends its run
  size_t bucket_of(int64_t key) const {
    const size_t mask = map_.size() - 1;
    size_t b = home(key);
    while (map_[b] >= 0 && key_[(size_t)map_[b]] != key) b = (b + 1) & mask;
    return b;
  }
  int64_t find(int64_t key) const { return map_[bucket_of(key)]; }

  int64_t insert_new(int64_t key) {
    if ((size_ + 1) * 4 > (int64_t)map_.size() * 3) rehash(map_.size() * 2);
    int64_t e;
    if (!free_.empty()) {
      e = free_.back();
      free_.pop_back();
    } else {
      e = (int64_t)key_.size();
      key_.push_back(0);
      version_.push_back(0);
      freq_.push_back(0);
      colmask_.push_back(0u);
      seen_.push_back(0);
      for (int c = 0; c < ncols(); ++c)
        slabs_[(size_t)c].resize(slabs_[(size_t)c].size() + (size_t)col_bytes_[(size_t)c]);
    }
    key_[(size_t)e] = key;
    for (int c = 0; c < ncols(); ++c) {
      const int64_t b = col_bytes_[(size_t)c];
      if (b) memset(&slabs_[(size_t)c][(size_t)(e * b)], 0, (size_t)b);
    }
    map_[bucket_of(key)] = e;
    ++size_;
    return e;
  }

  void rehash(size_t buckets) {
    std::vector<int64_t> old;
    old.swap(map_);
    map_.assign(buckets, -1);
    for (int64_t e : old)
      if (e >= 0) map_[bucket_of(key_[(size_t)e])] = e;
  }

  // Linear probing without tombstones: the entries of the run behind the hole
  // move back into it unless that would put them before their home bucket.
  void erase_entry(int64_t e) {
    const size_t mask = map_.size() - 1;
    size_t hole = bucket_of(key_[(size_t)e]);
    map_[hole] = -1;
    for (size_t j = (hole + 1) & mask; map_[j] >= 0; j = (j + 1) & mask) {
      const size_t h = home(key_[(size_t)map_[j]]);
      // the entry at j may move to the hole iff its home is not in (hole, j] cyclically
      if (((j - h) & mask) >= ((j - hole) & mask)) {
        map_[hole] = map_[j];
        map_[j] = -1;
        hole = j;
      }
    }
    free_.push_back(e);
    --size_;
  }

  void copy_out(int64_t e, int64_t j, void* const* values_out, int64_t* versions_out,
                int64_t* freqs_out, uint32_t* colmask_out) const {
    if (versions_out) versions_out[j] = version_[(size_t)e];
    if (freqs_out) freqs_out[j] = freq_[(size_t)e];
    if (colmask_out) colmask_out[j] = colmask_[(size_t)e];
    if (!values_out) return;
    for (int c = 0; c < ncols(); ++c) {
      const int64_t b = col_bytes_[(size_t)c];
      if (values_out[c] && b)
        memcpy(static_cast<char*>(values_out[c]) + j * b, &slabs_[(size_t)c][(size_t)(e * b)],
               (size_t)b);
    }
  }

  std::vector<int64_t> col_bytes_;
  std::vector<int64_t> map_;  // entry index per bucket, -1 = empty
  std::vector<int64_t> key_, version_, freq_;
  std::vector<uint32_t> colmask_;
  std::vector<uint8_t> seen_;  // per entry, set only inside take()
  std::vector<std::vector<uint8_t>> slabs_;
  std::vector<int64_t> free_, hit_;
  int64_t size_ = 0;
};

}  // namespace dr

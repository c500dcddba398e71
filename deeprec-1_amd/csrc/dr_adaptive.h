// dr_adaptive.h -- the bucket rule of an AdaptiveEmbeddingVariable: which row
// of the shared hash table an id trains while it has no row of its own in the
// EV.  Host and device share it; it has no dependency beyond <stdint.h>, so a
// stand-alone host program can check it (tools/adaptive_index_check.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DR_ADAPTIVE_HD __host__ __device__
#else
#define DR_ADAPTIVE_HD
#endif

// floormod(id, bucket_size) on int64 with floor semantics for negative ids
// (Python's %), bucket_size >= 1: always a valid row of the hash table.
DR_ADAPTIVE_HD static inline int64_t dr_adaptive_bucket(int64_t id, int64_t bucket_size) {
  if ((((uint64_t)id | (uint64_t)bucket_size) >> 32) == 0) {
    // both fit 32 unsigned bits: the same value, without the 64-bit division
    // (which a GPU emulates in dozens of instructions)
    return (int64_t)((uint32_t)id % (uint32_t)bucket_size);
  }
  int64_t r = id % bucket_size;  // sign of id
  if (r < 0) r += bucket_size;
  return r;
}

// A supplied bucket row (hash_ev_ids) is a valid row iff 0 <= h < bucket_size.
DR_ADAPTIVE_HD static inline bool dr_adaptive_row_valid(int64_t h, int64_t bucket_size) {
  return (uint64_t)h < (uint64_t)bucket_size;
}

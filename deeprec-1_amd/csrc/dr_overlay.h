// dr_overlay.h -- the search of the host-tier serving overlay (DESIGN
// section 19): the rows a read-only pooled lookup serves from the host-DRAM
// tier travel to the device as (ov_keys, ov_rows), the keys strictly
// ascending as signed int64 inside each table's range, and a lane finds its
// key there with a lower bound.
//
// Header-only and host-compilable (tests/test_overlay_search_host.py checks it
// against std::lower_bound on the CPU).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DR_OV_HD __host__ __device__
#else
#define DR_OV_HD
#endif

namespace dr {

// First index i in [lo, hi) with keys[i] >= key (signed), hi when there is
// none; lo >= hi (an empty range) returns lo.
DR_OV_HD inline int64_t overlay_lower_bound(const int64_t* keys, int64_t lo, int64_t hi,
                                            int64_t key) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// Index of `key` in the sorted range keys[lo, hi), or -1.
DR_OV_HD inline int64_t overlay_find(const int64_t* keys, int64_t lo, int64_t hi, int64_t key) {
  const int64_t i = overlay_lower_bound(keys, lo, hi, key);
  return i < hi && keys[i] == key ? i : -1;
}

}  // namespace dr

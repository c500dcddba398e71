// host_tier.hip -- C entries of the host-DRAM tier (dr_host_tier.h; DESIGN
// section 16).  Host code only: every pointer is a host pointer, no device is
// touched.  The caller serialises the calls on one tier (the Python layer
// holds the primary EV's lock around them).
#include <new>

#include "dr_common.h"
#include "dr_host_tier.h"

struct dr_host_tier {
  dr::HostTier t;
  dr_host_tier(int ncols, const int64_t* col_bytes, int64_t hint) : t(ncols, col_bytes, hint) {}
};

// A host allocation that fails is DR_RESOURCE_EXHAUSTED, not an exception
// through the C ABI.
#define DR_TIER_TRY(what, ...)                                                   \
  try {                                                                          \
    __VA_ARGS__;                                                                 \
  } catch (const std::bad_alloc&) {                                              \
    ::dr::set_error("%s: out of host memory", what);                             \
    return DR_RESOURCE_EXHAUSTED;                                                \
  }

extern "C" {

int dr_host_tier_create(int ncols, const int64_t* col_bytes, int64_t capacity_hint,
                        dr_host_tier** out) {
  DR_REQUIRE(out && col_bytes && ncols >= 1 && ncols <= 16, DR_INVALID_ARGUMENT,
             "dr_host_tier_create: 1..16 columns and their sizes");
  for (int c = 0; c < ncols; ++c)
    DR_REQUIRE(col_bytes[c] >= 0, DR_INVALID_ARGUMENT, "dr_host_tier_create: column %d has %lld B",
               c, (long long)col_bytes[c]);
  DR_REQUIRE(capacity_hint >= 0, DR_INVALID_ARGUMENT, "dr_host_tier_create: capacity_hint < 0");
  DR_TIER_TRY("dr_host_tier_create", *out = new dr_host_tier(ncols, col_bytes, capacity_hint));
  return DR_OK;
}

int dr_host_tier_destroy(dr_host_tier* t) {
  delete t;
  return DR_OK;
}

int dr_host_tier_size(dr_host_tier* t, int64_t* n) {
  DR_REQUIRE(t && n, DR_INVALID_ARGUMENT, "dr_host_tier_size: null argument");
  *n = t->t.size();
  return DR_OK;
}

int dr_host_tier_put(dr_host_tier* t, const int64_t* keys, int64_t n, const void* const* values,
                     const int64_t* versions, const int64_t* freqs, const uint32_t* colmask) {
  DR_REQUIRE(t && n >= 0 && (n == 0 || keys), DR_INVALID_ARGUMENT, "dr_host_tier_put: bad argument");
  DR_TIER_TRY("dr_host_tier_put", t->t.put(keys, n, values, versions, freqs, colmask));
  return DR_OK;
}

int dr_host_tier_take(dr_host_tier* t, const int64_t* keys, int64_t n, int erase,
                      int64_t* hit_index_out, void* const* values_out, int64_t* versions_out,
                      int64_t* freqs_out, uint32_t* colmask_out, int64_t* hits) {
  DR_REQUIRE(t && hits && n >= 0 && (n == 0 || keys), DR_INVALID_ARGUMENT,
             "dr_host_tier_take: bad argument");
  DR_TIER_TRY("dr_host_tier_take",
              *hits = t->t.take(keys, n, erase, hit_index_out, values_out, versions_out, freqs_out,
                                colmask_out));
  return DR_OK;
}

int dr_host_tier_remove(dr_host_tier* t, const int64_t* keys, int64_t n, int64_t* removed) {
  DR_REQUIRE(t && n >= 0 && (n == 0 || keys), DR_INVALID_ARGUMENT,
             "dr_host_tier_remove: bad argument");
  int64_t r = 0;
  DR_TIER_TRY("dr_host_tier_remove", r = t->t.remove(keys, n));
  if (removed) *removed = r;
  return DR_OK;
}

int dr_host_tier_shrink(dr_host_tier* t, int64_t global_step, int64_t steps_to_live,
                        int64_t* removed) {
  DR_REQUIRE(t, DR_INVALID_ARGUMENT, "dr_host_tier_shrink: null tier");
  int64_t r = 0;
  DR_TIER_TRY("dr_host_tier_shrink", r = t->t.shrink(global_step, steps_to_live));
  if (removed) *removed = r;
  return DR_OK;
}

int dr_host_tier_export(dr_host_tier* t, int64_t* keys_out, void* const* values_out,
                        int64_t* versions_out, int64_t* freqs_out, uint32_t* colmask_out,
                        int64_t capacity, int64_t* m) {
  DR_REQUIRE(t && m, DR_INVALID_ARGUMENT, "dr_host_tier_export: null argument");
  *m = t->t.size();
  if (!keys_out && !values_out && !versions_out && !freqs_out && !colmask_out) return DR_OK;
  DR_REQUIRE(capacity >= *m, DR_INVALID_ARGUMENT, "dr_host_tier_export: capacity %lld < %lld",
             (long long)capacity, (long long)*m);
  DR_TIER_TRY("dr_host_tier_export",
              t->t.export_all(keys_out, values_out, versions_out, freqs_out, colmask_out));
  return DR_OK;
}

// -- colmask as a flag word: the update bit of an incremental checkpoint
// travels in bit 16 (DR_TIER_UPDATED) -----------------------

int dr_host_tier_count_masked(dr_host_tier* t, uint32_t mask, int64_t* n) {
  DR_REQUIRE(t && n, DR_INVALID_ARGUMENT, "dr_host_tier_count_masked: null argument");
  *n = t->t.count_masked(mask);
  return DR_OK;
}

int dr_host_tier_export_masked(dr_host_tier* t, uint32_t mask, int64_t* keys_out,
                               void* const* values_out, int64_t* versions_out, int64_t* freqs_out,
                               uint32_t* colmask_out, int64_t capacity, int64_t* m) {
  DR_REQUIRE(t && m, DR_INVALID_ARGUMENT, "dr_host_tier_export_masked: null argument");
  *m = t->t.count_masked(mask);
  if (!keys_out && !values_out && !versions_out && !freqs_out && !colmask_out) return DR_OK;
  DR_REQUIRE(capacity >= *m, DR_INVALID_ARGUMENT,
             "dr_host_tier_export_masked: capacity %lld < %lld", (long long)capacity,
             (long long)*m);
  DR_TIER_TRY("dr_host_tier_export_masked",
              t->t.export_masked(mask, keys_out, values_out, versions_out, freqs_out, colmask_out));
  return DR_OK;
}

int dr_host_tier_clear_bits(dr_host_tier* t, uint32_t mask, int64_t* changed) {
  DR_REQUIRE(t, DR_INVALID_ARGUMENT, "dr_host_tier_clear_bits: null tier");
  const int64_t c = t->t.clear_bits(mask);
  if (changed) *changed = c;
  return DR_OK;
}

int dr_host_tier_or_bits(dr_host_tier* t, const int64_t* keys, int64_t n, uint32_t require,
                         uint32_t bits, int64_t* hit) {
  DR_REQUIRE(t && n >= 0 && (n == 0 || keys), DR_INVALID_ARGUMENT,
             "dr_host_tier_or_bits: bad argument");
  int64_t h = 0;
  DR_TIER_TRY("dr_host_tier_or_bits", h = t->t.or_bits(keys, n, require, bits));
  if (hit) *hit = h;
  return DR_OK;
}

int dr_host_tier_shrink_keys(dr_host_tier* t, int64_t global_step, int64_t steps_to_live,
                             int64_t* keys_out, int64_t capacity, int64_t* removed) {
  DR_REQUIRE(t, DR_INVALID_ARGUMENT, "dr_host_tier_shrink_keys: null tier");
  // refused before the walk stamps a version or drops a key
  DR_REQUIRE(capacity >= t->t.size() && (keys_out || t->t.size() == 0), DR_INVALID_ARGUMENT,
             "dr_host_tier_shrink_keys: capacity %lld < the tier's %lld keys", (long long)capacity,
             (long long)t->t.size());
  int64_t r = 0;
  DR_TIER_TRY("dr_host_tier_shrink_keys",
              r = t->t.shrink_keys(global_step, steps_to_live, keys_out));
  if (removed) *removed = r;
  return DR_OK;
}

}  // extern "C"

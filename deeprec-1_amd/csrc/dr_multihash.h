// dr_multihash.h -- the index rule of a MultiHashVariable ("Q-R",
// quotient-remainder): the one place that says which row of the Q table and
// which row of the R table an id selects.  Host and device share it; it has
// no dependency beyond <stdint.h>, so a stand-alone host program can check it
// (tools/multihash_index_check.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DR_MHV_HD __host__ __device__
#else
#define DR_MHV_HD
#endif

// Operation codes (how the two rows of an id are combined); the same values
// as in include/deeprec_amd.h.
#ifndef DR_MHV_ADD
#define DR_MHV_ADD 0    /* Q[q] + R[r]   (Dq == Dr) */
#define DR_MHV_MUL 1    /* Q[q] * R[r]   (Dq == Dr) */
#define DR_MHV_CONCAT 2 /* [Q[q] ; R[r]] (Dq + Dr columns) */
#endif

// q = floordiv(id, q_rows), r = floormod(id, r_rows) on int64 with floor
// semantics for negative ids (Python's // and %), q_rows >= 1, r_rows >= 1.
// The quotient's divisor is the Q table's row count.  r is always a valid
// row of R; q is a valid row of Q iff 0 <= q < q_rows (ids in
// [0, q_rows * q_rows)), which the callers check.
DR_MHV_HD static inline void dr_mhv_index(int64_t id, int64_t q_rows, int64_t r_rows, int64_t* q,
                                          int64_t* r) {
  if ((((uint64_t)id | (uint64_t)q_rows | (uint64_t)r_rows) >> 32) == 0) {
    // everything fits 32 unsigned bits: the same values, without the 64-bit
    // division (which a GPU emulates in dozens of instructions)
    *q = (int64_t)((uint32_t)id / (uint32_t)q_rows);
    *r = (int64_t)((uint32_t)id % (uint32_t)r_rows);
    return;
  }
  int64_t qq = id / q_rows;  // truncates toward zero
  if (id < 0 && qq * q_rows != id) --qq;
  int64_t rr = id % r_rows;  // sign of id
  if (rr < 0) rr += r_rows;
  *q = qq;
  *r = rr;
}

DR_MHV_HD static inline bool dr_mhv_q_valid(int64_t q, int64_t q_rows) {
  return (uint64_t)q < (uint64_t)q_rows;
}

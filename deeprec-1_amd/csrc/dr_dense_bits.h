// dr_dense_bits.h -- the update marks of a dense table: one bit per row in
// ceil(rows / 32) uint32 words, bit (row & 31) of word (row >> 5).  The bits of
// the last word at or past `rows` are never set by the library and are masked
// off wherever the words are read.  Host and device share the arithmetic; it
// has no dependency beyond <stdint.h>, so a stand-alone host program can check
// it (tools/dense_bits_check.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DR_DENSE_BITS_HD __host__ __device__
#else
#define DR_DENSE_BITS_HD
#endif

// Number of words that hold the marks of `rows` rows (0 for rows <= 0).
DR_DENSE_BITS_HD static inline int64_t dr_dense_bits_words(int64_t rows) {
  return rows <= 0 ? 0 : ((rows - 1) >> 5) + 1;
}

// Word index and mask of row `row` (row >= 0).
DR_DENSE_BITS_HD static inline int64_t dr_dense_bits_word(int64_t row) { return row >> 5; }
DR_DENSE_BITS_HD static inline uint32_t dr_dense_bits_mask(int64_t row) {
  return (uint32_t)1 << (uint32_t)(row & 31);
}

// The valid bits of the LAST word of a table of `rows` rows (rows >= 1).
DR_DENSE_BITS_HD static inline uint32_t dr_dense_bits_tail_mask(int64_t rows) {
  const uint32_t r = (uint32_t)(rows & 31);
  return r ? (((uint32_t)1 << r) - 1u) : 0xFFFFFFFFu;
}

// The valid bits of word `w` of a table of `rows` rows: all of them except in
// the last word; nothing at or past the last word's end.
DR_DENSE_BITS_HD static inline uint32_t dr_dense_bits_valid(int64_t w, int64_t rows) {
  const int64_t nw = dr_dense_bits_words(rows);
  if (w < 0 || w >= nw) return 0u;
  return w == nw - 1 ? dr_dense_bits_tail_mask(rows) : 0xFFFFFFFFu;
}

DR_DENSE_BITS_HD static inline int dr_dense_bits_popcount(uint32_t x) {
  x = x - ((x >> 1) & 0x55555555u);
  x = (x & 0x33333333u) + ((x >> 2) & 0x33333333u);
  x = (x + (x >> 4)) & 0x0F0F0F0Fu;
  return (int)((x * 0x01010101u) >> 24);
}

// Rank of bit `bit` (0 .. 31) inside `word`: the number of set bits below it,
// i.e. the place of that row among the word's marked rows in ascending order.
DR_DENSE_BITS_HD static inline int dr_dense_bits_rank(uint32_t word, int bit) {
  return dr_dense_bits_popcount(word & (((uint32_t)1 << (uint32_t)(bit & 31)) - 1u));
}

// Host check of the dense update-mark arithmetic (deeprec-1_amd/csrc/
// dr_dense_bits.h): reads "row word_value" pairs from stdin (int64 row, uint32
// word contents in decimal), one per line, and prints for each
//   row  word_index  mask  rank  valid_mask_of_that_word
// for a table of ROWS rows, after one header line "words tail_mask".  rank is
// the rank of the row's bit inside the given word contents.  The caller
// (tests/test_dense_bits_host.py) compares with Python integers.
//   g++ -O2 -std=c++17 -I deeprec-1_amd/csrc tools/dense_bits_check.cpp
//   ./a.out ROWS < pairs.txt
// (also builds with -fsanitize=address,undefined)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "dr_dense_bits.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s ROWS < pairs\n", argv[0]);
    return 2;
  }
  const int64_t rows = std::strtoll(argv[1], nullptr, 10);
  if (rows < 1) {
    std::fprintf(stderr, "rows must be >= 1\n");
    return 2;
  }
  std::printf("%" PRId64 " %" PRIu32 "\n", dr_dense_bits_words(rows),
              dr_dense_bits_tail_mask(rows));
  int64_t row;
  uint32_t word;
  while (std::scanf("%" SCNd64 " %" SCNu32, &row, &word) == 2) {
    if (row < 0) {
      std::fprintf(stderr, "rows are >= 0\n");
      return 2;
    }
    const int64_t w = dr_dense_bits_word(row);
    std::printf("%" PRId64 " %" PRId64 " %" PRIu32 " %d %" PRIu32 "\n", row, w,
                dr_dense_bits_mask(row), dr_dense_bits_rank(word, (int)(row & 31)),
                dr_dense_bits_valid(w, rows));
  }
  return 0;
}

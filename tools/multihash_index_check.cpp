// Host check of the MultiHashVariable index rule (deeprec-1_amd/csrc/
// dr_multihash.h): reads int64 ids from stdin, one per line, and prints
// "id q r valid" for each with the helper the kernels use.  The caller
// (tests/test_multihash_index_host.py) compares with Python's // and %.
//   g++ -O2 -std=c++17 -I deeprec-1_amd/csrc tools/multihash_index_check.cpp
//   ./a.out Q_ROWS R_ROWS < ids.txt
// (also builds with -fsanitize=address,undefined)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "dr_multihash.h"

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s Q_ROWS R_ROWS < ids\n", argv[0]);
    return 2;
  }
  const int64_t q_rows = std::strtoll(argv[1], nullptr, 10);
  const int64_t r_rows = std::strtoll(argv[2], nullptr, 10);
  if (q_rows < 1 || r_rows < 1) {
    std::fprintf(stderr, "rows must be >= 1\n");
    return 2;
  }
  int64_t id;
  while (std::scanf("%" SCNd64, &id) == 1) {
    int64_t q, r;
    dr_mhv_index(id, q_rows, r_rows, &q, &r);
    std::printf("%" PRId64 " %" PRId64 " %" PRId64 " %d\n", id, q, r,
                (int)dr_mhv_q_valid(q, q_rows));
  }
  return 0;
}

// Host check of the AdaptiveEmbeddingVariable bucket rule (deeprec-1_amd/csrc/
// dr_adaptive.h): reads int64 values from stdin, one per line, and prints
// "value bucket valid" for each -- the bucket row the kernels derive from the
// value as an id, and whether the value itself would be accepted as a supplied
// bucket row.  The caller (tests/test_adaptive_index_host.py) compares with
// Python's %.
//   g++ -O2 -std=c++17 -I deeprec-1_amd/csrc tools/adaptive_index_check.cpp
//   ./a.out BUCKET_SIZE < ids.txt
// (also builds with -fsanitize=address,undefined)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "dr_adaptive.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s BUCKET_SIZE < ids\n", argv[0]);
    return 2;
  }
  const int64_t bucket_size = std::strtoll(argv[1], nullptr, 10);
  if (bucket_size < 1) {
    std::fprintf(stderr, "bucket_size must be >= 1\n");
    return 2;
  }
  int64_t id;
  while (std::scanf("%" SCNd64, &id) == 1) {
    std::printf("%" PRId64 " %" PRId64 " %d\n", id, dr_adaptive_bucket(id, bucket_size),
                (int)dr_adaptive_row_valid(id, bucket_size));
  }
  return 0;
}

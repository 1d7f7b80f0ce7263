// mismatch_tests.cpp — cs::FMIndex::count_mismatches through the drop-in header
// (include/cs/fm_index.hpp) and libcs_fmindex.so.  Expected values are the oracle's sums
// for "banana$": hist[d] = the summed exact counts of every string over {$, a, b, n} at
// Hamming distance d from the pattern (tests/test_zz_gpu_mismatch.py expected_hist).
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "cs/fm_index.hpp"

using namespace cs;
using H = std::vector<uint64_t>;

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

int main() {
  FMIndex idx = FMIndex::build_from_text("banana$", BuildParams{});
  CHECK((idx.count_mismatches("ana", 0) == H{2}));
  CHECK((idx.count_mismatches("ana", 1) == H{2, 0}));
  CHECK((idx.count_mismatches("ana", 3) == H{2, 0, 2, 3}));
  CHECK((idx.count_mismatches("nan", 1) == H{1, 2}));
  CHECK((idx.count_mismatches("bnn", 2) == H{0, 1, 3}));
  CHECK((idx.count_mismatches("banana", 2) == H{1, 0, 0}));
  CHECK((idx.count_mismatches("", 2) == H{7, 0, 0}));          // count("") = n
  CHECK((idx.count_mismatches("x", 1) == H{0, 7}));            // a byte absent from the text
  CHECK((idx.count_mismatches("a", 3) == H{3, 4, 0, 0}));      // shorter than k
  CHECK((idx.count_mismatches("banana$ba", 2) == H{1, 0, 0}));  // longer than the text: cyclic
  CHECK(idx.count_mismatches("ana", 1)[0] == idx.count("ana"));
  bool threw = false;
  try {
    (void)idx.count_mismatches("ana", 4);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);
  FMIndex none;  // an empty index, as count()
  CHECK((none.count_mismatches("a", 1) == H{0, 0}));
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("PASSED\n");
  return 0;
}

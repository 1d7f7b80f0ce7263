// best_mismatch_tests.cpp — cs::FMIndex::best_mismatch through the drop-in header
// (include/cs/fm_index.hpp) and libcs_fmindex.so.  Expected values are hard-coded from the
// oracle's sums (tests/helpers/mismatch_ref.py expected_hist, then the first non-zero column up
// to k: tests/helpers/best_ref.py best_from_hist) for "banana$" and a 21-symbol DNA text.
#include <cstdio>
#include <stdexcept>
#include <string>
#include <utility>

#include "cs/fm_index.hpp"

using namespace cs;
using B = std::pair<int, uint64_t>;

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

int main() {
  const B none{-1, 0};
  FMIndex idx = FMIndex::build_from_text("banana$", BuildParams{});
  for (unsigned k = 0; k <= 3; ++k) {
    CHECK((idx.best_mismatch("ana", k) == B{0, 2}));
    CHECK((idx.best_mismatch("nan", k) == B{0, 1}));
    CHECK((idx.best_mismatch("", k) == B{0, 7}));            // count("") = n
    CHECK((idx.best_mismatch("a", k) == B{0, 3}));           // shorter than k
    CHECK((idx.best_mismatch("banana$ba", k) == B{0, 1}));   // longer than the text: cyclic
    CHECK((idx.best_mismatch("bnn", k) == (k >= 1 ? B{1, 1} : none)));
    CHECK((idx.best_mismatch("x", k) == (k >= 1 ? B{1, 7} : none)));  // a byte absent from the text
    CHECK((idx.best_mismatch("xx", k) == (k >= 2 ? B{2, 7} : none)));
    CHECK((idx.best_mismatch("nnnn", k) == (k >= 2 ? B{2, 2} : none)));
    CHECK((idx.best_mismatch("xxx", k) == (k >= 3 ? B{3, 7} : none)));
    CHECK((idx.best_mismatch("bbbb", k) == (k >= 3 ? B{3, 4} : none)));
    CHECK((idx.best_mismatch("bbbbb", k) == none));
    CHECK((idx.best_mismatch("xxxx", k) == none));           // d > m never resolves
  }
  CHECK(idx.best_mismatch("ana", 1).second == idx.count("ana"));
  CHECK(idx.best_mismatch("bnn", 2).second == idx.count_mismatches("bnn", 2)[1]);

  FMIndex dna = FMIndex::build_from_text("ACGTTGCAACGGTACCATGA$", BuildParams{});
  for (unsigned k = 0; k <= 3; ++k) {
    CHECK((dna.best_mismatch("ACGT", k) == B{0, 1}));
    CHECK((dna.best_mismatch("ACGTTGCAACGGTACCATGA", k) == B{0, 1}));
    CHECK((dna.best_mismatch("ACGATGCA", k) == (k >= 1 ? B{1, 1} : none)));
    CHECK((dna.best_mismatch("ACNT", k) == (k >= 1 ? B{1, 1} : none)));
    CHECK((dna.best_mismatch("TCGATGCA", k) == (k >= 2 ? B{2, 1} : none)));
    CHECK((dna.best_mismatch("TCGATGCT", k) == (k >= 3 ? B{3, 1} : none)));
    CHECK((dna.best_mismatch("ACCTTGGAACGCTACCATGA", k) == (k >= 3 ? B{3, 1} : none)));
    CHECK((dna.best_mismatch("ACCTTGGAAGGCTACCATGA", k) == none));
    CHECK((dna.best_mismatch("GGGGGGGG", k) == none));
    CHECK((dna.best_mismatch("", k) == B{0, 21}));
  }

  bool threw = false;
  try {
    (void)idx.best_mismatch("ana", 4);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);
  FMIndex empty;  // an empty index, as count()
  CHECK((empty.best_mismatch("a", 1) == none));
  CHECK((empty.best_mismatch("", 1) == none));  // n = 0 gives none
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("PASSED\n");
  return 0;
}

// best_locate_tests.cpp — cs::FMIndex::locate_best_mismatch through the drop-in header
// (include/cs/fm_index.hpp) and libcs_fmindex.so.  Expected values are hard-coded from the
// oracle's enumeration (tests/helpers/mismatch_ref.py expected_hist and expected_pairs, then
// tests/helpers/best_locate_ref.py best_pairs) for "banana$" and a 21-symbol DNA text; the
// positions are compared sorted.
#include <algorithm>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "cs/fm_index.hpp"

using namespace cs;
using V = std::vector<uint64_t>;
using R = std::pair<int, V>;

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

static R sorted(R r) {
  std::sort(r.second.begin(), r.second.end());
  return r;
}

int main() {
  const R none{-1, {}};
  const V all7{0, 1, 2, 3, 4, 5, 6};
  FMIndex idx = FMIndex::build_from_text("banana$", BuildParams{});
  for (unsigned k = 0; k <= 3; ++k) {
    CHECK((sorted(idx.locate_best_mismatch("ana", k)) == R{0, {1, 3}}));
    CHECK((sorted(idx.locate_best_mismatch("nan", k)) == R{0, {2}}));
    CHECK((sorted(idx.locate_best_mismatch("", k)) == R{0, {}}));  // locate("") is empty, count("") = n
    CHECK((sorted(idx.locate_best_mismatch("a", k)) == R{0, {1, 3, 5}}));   // shorter than k
    CHECK((sorted(idx.locate_best_mismatch("banana$ba", k)) == R{0, {0}}));  // longer than the text: cyclic
    CHECK((sorted(idx.locate_best_mismatch("bnn", k)) == (k >= 1 ? R{1, {0}} : none)));
    CHECK((sorted(idx.locate_best_mismatch("x", k)) == (k >= 1 ? R{1, all7} : none)));  // a byte absent from the text
    CHECK((sorted(idx.locate_best_mismatch("xx", k)) == (k >= 2 ? R{2, all7} : none)));
    CHECK((sorted(idx.locate_best_mismatch("nnnn", k)) == (k >= 2 ? R{2, {1, 2}} : none)));
    CHECK((sorted(idx.locate_best_mismatch("xxx", k)) == (k >= 3 ? R{3, all7} : none)));
    CHECK((sorted(idx.locate_best_mismatch("bbbb", k)) == (k >= 3 ? R{3, {0, 4, 5, 6}} : none)));
    CHECK((sorted(idx.locate_best_mismatch("bbbbb", k)) == none));
    CHECK((sorted(idx.locate_best_mismatch("xxxx", k)) == none));  // d > m never resolves
  }
  // k = 0 is the exact locate, element for element; the distance and the size are best_mismatch's
  CHECK(idx.locate_best_mismatch("ana", 0).second == idx.locate("ana"));
  CHECK(idx.locate_best_mismatch("a", 0).second == idx.locate("a"));
  for (const char* p : {"ana", "bnn", "xx", "bbbb", "bbbbb"}) {
    const auto b = idx.best_mismatch(p, 3);
    const auto l = idx.locate_best_mismatch(p, 3);
    CHECK(l.first == b.first && l.second.size() == b.second);
  }

  FMIndex dna = FMIndex::build_from_text("ACGTTGCAACGGTACCATGA$", BuildParams{});
  for (unsigned k = 0; k <= 3; ++k) {
    CHECK((sorted(dna.locate_best_mismatch("ACGT", k)) == R{0, {0}}));
    CHECK((sorted(dna.locate_best_mismatch("A", k)) == R{0, {0, 7, 8, 13, 16, 19}}));
    CHECK((sorted(dna.locate_best_mismatch("AC", k)) == R{0, {0, 8, 13}}));
    CHECK((sorted(dna.locate_best_mismatch("ACGATGCA", k)) == (k >= 1 ? R{1, {0}} : none)));
    CHECK((sorted(dna.locate_best_mismatch("ACNT", k)) == (k >= 1 ? R{1, {0}} : none)));
    CHECK((sorted(dna.locate_best_mismatch("NC", k)) == (k >= 1 ? R{1, {0, 5, 8, 13, 14}} : none)));  // five leaves
    CHECK((sorted(dna.locate_best_mismatch("TCGATGCA", k)) == (k >= 2 ? R{2, {0}} : none)));
    CHECK((sorted(dna.locate_best_mismatch("ANNT", k)) == (k >= 2 ? R{2, {0}} : none)));
    CHECK((sorted(dna.locate_best_mismatch("TCGATGCT", k)) == (k >= 3 ? R{3, {0}} : none)));
    CHECK((sorted(dna.locate_best_mismatch("GGGGGGGG", k)) == none));
    CHECK((sorted(dna.locate_best_mismatch("", k)) == R{0, {}}));
  }

  bool threw = false;
  try {
    (void)idx.locate_best_mismatch("ana", 4);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);
  FMIndex empty;  // an empty index, as best_mismatch()
  CHECK((empty.locate_best_mismatch("a", 1) == none));
  CHECK((empty.locate_best_mismatch("", 1) == none));  // n = 0 gives none
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("PASSED\n");
  return 0;
}

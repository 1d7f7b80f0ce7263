// mismatch_locate_tests.cpp — cs::FMIndex::locate_mismatches through the drop-in header
// (include/cs/fm_index.hpp) and libcs_fmindex.so.  Expected values are the oracle's: the union,
// over every string S over the text's symbols at Hamming distance d <= k from the pattern, of
// the exact locate of S labelled d (tests/test_zz_gpu_mismatch_locate.py expected_pairs),
// for "banana$" and for 400 bases from a linear congruential generator with a terminator.
// The order inside a result is the search's, so results are compared sorted.
#include <algorithm>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "cs/fm_index.hpp"

using namespace cs;
using PD = std::vector<std::pair<uint64_t, uint8_t>>;

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

static PD sorted(PD v) {
  std::sort(v.begin(), v.end());
  return v;
}

int main() {
  FMIndex idx = FMIndex::build_from_text("banana$", BuildParams{});
  CHECK((sorted(idx.locate_mismatches("ana", 0)) == PD{{1, 0}, {3, 0}}));
  CHECK((sorted(idx.locate_mismatches("ana", 1)) == PD{{1, 0}, {3, 0}}));
  CHECK((sorted(idx.locate_mismatches("ana", 3)) ==
         PD{{0, 3}, {1, 0}, {2, 3}, {3, 0}, {4, 3}, {5, 2}, {6, 2}}));
  CHECK((sorted(idx.locate_mismatches("nan", 1)) == PD{{0, 1}, {2, 0}, {4, 1}}));
  CHECK((sorted(idx.locate_mismatches("bnn", 2)) == PD{{0, 1}, {1, 2}, {2, 2}, {3, 2}}));
  CHECK((sorted(idx.locate_mismatches("banana", 2)) == PD{{0, 0}}));
  CHECK(idx.locate_mismatches("", 2).empty());  // locate("") = {}
  CHECK((sorted(idx.locate_mismatches("x", 1)) ==  // a byte absent from the text
         PD{{0, 1}, {1, 1}, {2, 1}, {3, 1}, {4, 1}, {5, 1}, {6, 1}}));
  CHECK((sorted(idx.locate_mismatches("a", 3)) ==  // shorter than k
         PD{{0, 1}, {1, 0}, {2, 1}, {3, 0}, {4, 1}, {5, 0}, {6, 1}}));
  CHECK((sorted(idx.locate_mismatches("banana$ba", 2)) == PD{{0, 0}}));  // longer than the text: cyclic
  {  // k = 0 is the exact locate, order included
    const std::vector<uint64_t> exact = idx.locate("ana");
    const PD got = idx.locate_mismatches("ana", 0);
    CHECK(got.size() == exact.size());
    for (size_t i = 0; i < got.size() && i < exact.size(); ++i) CHECK(got[i].first == exact[i] && got[i].second == 0);
  }
  {  // the sizes are the count's histogram row sums
    const std::vector<uint64_t> hist = idx.count_mismatches("ana", 3);
    CHECK(hist[0] + hist[1] + hist[2] + hist[3] == idx.locate_mismatches("ana", 3).size());
  }
  bool threw = false;
  try {
    (void)idx.locate_mismatches("ana", 4);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);
  FMIndex none;  // an empty index, as locate()
  CHECK(none.locate_mismatches("a", 1).empty());

  std::string dna;
  uint32_t x = 12345;
  for (int i = 0; i < 400; ++i) {
    x = (x * 1103515245u + 12345u) & 0x7FFFFFFFu;
    dna.push_back("ACGT"[(x >> 16) & 3]);
  }
  CHECK(dna.substr(0, 12) == "AACGTCCGGCAT");
  dna.push_back('$');
  FMIndex d = FMIndex::build_from_text(dna, BuildParams{});
  CHECK(d.locate_mismatches("ACGGAATGAGGC", 0).empty());  // text[100, 112) with one base replaced
  CHECK((sorted(d.locate_mismatches("ACGGAATGAGGC", 1)) == PD{{100, 1}}));
  CHECK((sorted(d.locate_mismatches("ACGGAATGAGGC", 2)) == PD{{100, 1}}));
  CHECK((sorted(d.locate_mismatches("ACTCGA", 1)) == PD{{200, 0}, {288, 0}, {357, 1}}));
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("PASSED\n");
  return 0;
}

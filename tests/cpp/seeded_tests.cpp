// seeded_tests.cpp — the seeded locate (include/cs_fmindex_approx_seeded.h) through the drop-in
// header's cs::FMIndex::locate_mismatches_seeded and through the C ABI, linked to
// libcs_fmindex.so.  Expected values are computed here by a plain loop: the Hamming distance of
// the pattern to the cyclic window at every start of a text with a unique smallest last byte
// (800 bases from a linear congruential generator, two planted copies of the pattern's source
// with substitutions, and a terminator).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "cs/fm_index.hpp"
#include "cs_fmindex.h"
#include "cs_fmindex_approx_seeded.h"
#include "cs_fmindex_tuning.h"

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

// every (start, distance) with distance <= k on the cyclic text, by position
static PD scan(const std::string& text, const std::string& pat, unsigned k) {
  PD out;
  const size_t n = text.size(), m = pat.size();
  for (size_t i = 0; i < n; ++i) {
    unsigned d = 0;
    for (size_t j = 0; j < m; ++j) d += text[(i + j) % n] != pat[j];
    if (d <= k) out.emplace_back(i, (uint8_t)d);
  }
  return out;
}

int main() {
  std::string dna;
  uint32_t x = 12345;
  for (int i = 0; i < 800; ++i) {
    x = (x * 1103515245u + 12345u) & 0x7FFFFFFFu;
    dna.push_back("ACGT"[(x >> 16) & 3]);
  }
  // a second copy of text[100, 160) at 500 with four substitutions, a third at 650 with six
  for (int j = 0; j < 60; ++j) dna[500 + j] = dna[100 + j], dna[650 + j] = dna[100 + j];
  for (int j : {3, 17, 30, 58}) dna[500 + j] = dna[500 + j] == 'A' ? 'C' : 'A';
  for (int j : {0, 9, 21, 33, 45, 59}) dna[650 + j] = dna[650 + j] == 'G' ? 'T' : 'G';
  dna.push_back('$');
  std::string pat = dna.substr(100, 60);
  pat[40] = pat[40] == 'T' ? 'G' : 'T';  // the source itself is at distance 1

  FMIndex idx = FMIndex::build_from_text(dna, BuildParams{});
  const PD want5 = scan(dna, pat, 5);
  CHECK(want5.size() == 2 && want5[0] == std::make_pair(uint64_t(100), uint8_t(1)) &&
        want5[1] == std::make_pair(uint64_t(500), uint8_t(5)));
  CHECK(sorted(idx.locate_mismatches_seeded(pat, 5)) == want5);
  CHECK(sorted(idx.locate_mismatches_seeded(pat, 7)) == scan(dna, pat, 7));  // the third copy, d = 7
  CHECK(scan(dna, pat, 7).size() == 3);
  CHECK(idx.locate_mismatches_seeded(pat, 0).empty());
  CHECK(sorted(idx.locate_mismatches_seeded(pat, 3)) == sorted(idx.locate_mismatches(pat, 3)));
  {  // a window through the end of the text and a pattern longer than the text
    const std::string wrap = dna.substr(dna.size() - 20) + dna.substr(0, 25);
    CHECK(sorted(idx.locate_mismatches_seeded(wrap, 5)) == scan(dna, wrap, 5));
    const std::string lng = dna + dna.substr(0, 7);
    CHECK(sorted(idx.locate_mismatches_seeded(lng, 5)) == scan(dna, lng, 5));
    CHECK(scan(dna, lng, 5).size() == 1);
  }
  {  // k = 0 is the exact locate, order included
    const std::string p = dna.substr(100, 6);
    const std::vector<uint64_t> exact = idx.locate(p);
    const PD got = idx.locate_mismatches_seeded(p, 0);
    CHECK(got.size() == exact.size() && !exact.empty());
    for (size_t i = 0; i < got.size() && i < exact.size(); ++i) CHECK(got[i].first == exact[i] && got[i].second == 0);
  }
  CHECK(idx.locate_mismatches_seeded("", 2).empty());
  FMIndex none;  // an empty index, as locate_mismatches()
  CHECK(none.locate_mismatches_seeded("ACGT", 1).empty());

  bool threw = false;
  try {
    (void)idx.locate_mismatches_seeded(pat, 16);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);
  threw = false;
  try {  // a pattern not longer than k
    (void)idx.locate_mismatches_seeded("ACG", 3);
  } catch (const std::runtime_error& e) {
    threw = std::strstr(e.what(), "pattern 0") != nullptr;
  }
  CHECK(threw);

  // the C ABI: sizing call, capacity, candidates
  const uint8_t* pp = reinterpret_cast<const uint8_t*>(pat.data());
  {
    uint64_t nout = 77;
    CHECK(cs_fm_locate_mismatch_seeded(idx.handle(), pp, pat.size(), 5, nullptr, nullptr, 0, &nout) ==
          CS_ERR_CAPACITY);
    CHECK(nout == 2);
    uint64_t pos[3] = {9, 9, 9};
    uint8_t dist[3] = {9, 9, 9};
    CHECK(cs_fm_locate_mismatch_seeded(idx.handle(), pp, pat.size(), 5, pos, dist, 1, &nout) == CS_ERR_CAPACITY);
    CHECK(nout == 2 && pos[0] == 9 && dist[0] == 9);  // untouched
    CHECK(cs_fm_locate_mismatch_seeded(idx.handle(), pp, pat.size(), 5, pos, dist, 2, &nout) == CS_OK);
    CHECK(nout == 2 && pos[2] == 9 && dist[2] == 9);
    PD got{{pos[0], dist[0]}, {pos[1], dist[1]}};
    CHECK(sorted(got) == want5);
    const uint64_t offs[2] = {0, pat.size()};
    uint64_t oo[2] = {9, 9}, total = 9, cand = 9;
    CHECK(cs_fm_locate_mismatch_seeded_batch(idx.handle(), pp, offs, 1, 5, oo, pos, dist, 3, &total, &cand,
                                             nullptr) == CS_OK);
    CHECK(total == 2 && oo[0] == 0 && oo[1] == 2 && cand >= 2);
    CHECK(cs_fm_locate_mismatch_seeded(idx.handle(), pp, pat.size(), 16, pos, dist, 3, &nout) == CS_ERR_INVALID);
    CHECK(cs_fm_locate_mismatch_seeded(idx.handle(), pp, 5, 5, pos, dist, 3, &nout) == CS_ERR_INVALID);
    CHECK(std::strstr(cs_fm_last_error(), "pattern 0") != nullptr);
    CHECK(cs_fm_locate_mismatch_seeded(nullptr, pp, pat.size(), 5, pos, dist, 3, &nout) == CS_ERR_INVALID);
    CHECK(std::strstr(cs_fm_last_error(), "null index handle") != nullptr);
  }

  // CS_ERR_UNSUPPORTED: no unique smallest last byte; no byte text in HBM
  {
    cs_build_params bp;
    cs_default_build_params(&bp);
    uint64_t pos[4] = {9, 9, 9, 9}, nout = 9;
    uint8_t dist[4] = {9, 9, 9, 9};
    cs_fm_index* h = nullptr;
    CHECK(cs_fm_build_from_text(reinterpret_cast<const uint8_t*>("abab"), 4, &bp, 0, &h) == CS_OK);
    if (h) {
      CHECK(cs_fm_locate_mismatch_seeded(h, reinterpret_cast<const uint8_t*>("ab"), 2, 1, pos, dist, 4, &nout) ==
            CS_ERR_UNSUPPORTED);
      CHECK(std::strstr(cs_fm_last_error(), "smallest last symbol") != nullptr);
      cs_fm_destroy(h);
    }
    h = nullptr;
    CHECK(cs_fm_build_with_options(reinterpret_cast<const uint8_t*>(dna.data()), dna.size(), 0, &bp,
                                   "DEVICE_TEXT=0", 0, &h) == CS_OK);
    if (h) {
      CHECK(cs_fm_locate_mismatch_seeded(h, pp, pat.size(), 5, pos, dist, 4, &nout) == CS_ERR_UNSUPPORTED);
      CHECK(std::strstr(cs_fm_last_error(), "text in HBM") != nullptr);
      cs_fm_destroy(h);
    }
    CHECK(nout == 9 && pos[0] == 9 && dist[0] == 9);  // nothing written
  }

  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("PASSED\n");
  return 0;
}

/*
 * cs_fmindex_approx.h — approximate count: occurrences within k mismatches, per distance.
 *
 * For a pattern P of length m and a bound k <= CS_MM_MAX the result is a histogram of k + 1
 * uint64 values:
 *
 *     hist[d] = sum of count(S) over all byte strings S with |S| = m and Hamming(S, P) = d
 *
 * for d = 0..k, where count is the exact count of include/cs_fmindex.h (the reference's
 * FMIndex::count, src/api/fm_index.cpp:79-101, quirks included: a cyclic BWT, a symbol absent
 * from the text gives 0).  So hist[0] is the exact count of P; only symbols present in the text
 * contribute (the terminator and rare symbols among them); m = 0 gives hist[0] = n and zeros
 * after it; n = 0 gives zeros; d > m gives 0.  There is no cap on m.  A batch result is laid
 * out [npat][k + 1], row-major.
 *
 * The search is a depth-first backtracking search over the index (one pattern per GPU lane),
 * not an enumeration of the neighbours: the neighbours of a pattern share every suffix they
 * have in common.
 */
#ifndef CS_FMINDEX_APPROX_H
#define CS_FMINDEX_APPROX_H

#include <stdint.h>

#include "cs_fmindex.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the largest mismatch bound k; a larger one is CS_ERR_INVALID */
#define CS_MM_MAX 3u

/* Device batch, asynchronous on stream.  Pattern layout exactly as the exact device count's:
 * CSR offsets d_offs[npat + 1] into d_pats (unchecked), or d_offs == NULL for npat patterns of
 * fixed_m bytes back to back; d_pats may be NULL when every pattern is empty.  d_hist
 * receives npat * (k + 1) uint64.  flags: the CS_Q_* structure flags with their meaning there
 * (they only restrict what may be read and never change results).  Allocates no memory, needs
 * no workspace and reads no environment. */
cs_status cs_fm_count_mismatch_device(const cs_fm_index* h, const uint8_t* d_pats,
                                      const uint64_t* d_offs, uint64_t fixed_m, uint64_t npat,
                                      uint32_t k, uint64_t* d_hist, uint32_t flags, void* stream);

/* Host batch (pattern q = pats[offs[q] .. offs[q + 1]), offsets non-decreasing, else
 * CS_ERR_INVALID), staged through HBM; out_hist receives npat * (k + 1) uint64.  Synchronises
 * before returning.  One staged copy per call: the search, not the transfer, dominates a
 * mismatch batch (a 20-mer at k = 2 stands for 1,771 exact counts), so the chunked
 * page-locking of the exact host batch is not repeated here. */
cs_status cs_fm_count_mismatch_batch(const cs_fm_index* h, const uint8_t* pats,
                                     const uint64_t* offs, uint64_t npat, uint32_t k,
                                     uint64_t* out_hist, void* stream);

/* One pattern, host: out_hist receives k + 1 uint64. */
cs_status cs_fm_count_mismatch(const cs_fm_index* h, const uint8_t* pattern, uint64_t m,
                               uint32_t k, uint64_t* out_hist);

#ifdef __cplusplus
}
#endif
#endif /* CS_FMINDEX_APPROX_H */

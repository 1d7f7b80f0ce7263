/*
 * cs_fmindex_approx_best.h — best stratum: the smallest mismatch distance at which a pattern
 * occurs, and its count.  The companion of cs_fmindex_approx.h's histogram for the caller who
 * asks "how close does this pattern come, and how many hits are there?" first.
 *
 * For a pattern P and a bound k <= CS_MM_MAX, with hist the histogram of cs_fmindex_approx.h:
 *
 *     best_dist  = the smallest d <= k with hist[d] > 0      (uint8; CS_MM_NONE when none)
 *     best_count = hist[best_dist]                           (uint64; 0 when none)
 *
 * Every quirk of the histogram is inherited: m = 0 gives (0, n); n = 0 gives none; a symbol
 * absent from the text never counts; d > m never resolves; k = 0 is the exact count, with
 * CS_MM_NONE where that is 0.  best_count equals column best_dist of the histogram at any
 * bound >= best_dist.
 *
 * The search runs in rounds d = 0..k (one kernel each, back to back on the stream): round d
 * searches, at exactly d mismatches, the patterns that had no hit below d, packed densely.  A
 * pattern stops at its first distance with a hit, and the deep rounds' waves hold only
 * patterns that need them.
 */
#ifndef CS_FMINDEX_APPROX_BEST_H
#define CS_FMINDEX_APPROX_BEST_H

#include <stdint.h>

#include "cs_fmindex.h"
#include "cs_fmindex_approx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* best_dist of a pattern that does not occur within k mismatches */
#define CS_MM_NONE 0xFFu

/* Device batch, asynchronous on stream; never synchronises the host (but for the check of a
 * NULL d_pats against the offsets' ends, as the count's call).  Pattern layout and
 * flags exactly as cs_fm_count_mismatch_device's: CSR offsets d_offs[npat + 1] into d_pats
 * (unchecked), or d_offs == NULL for npat patterns of fixed_m bytes back to back; d_pats may
 * be NULL when every pattern is empty; the CS_Q_* structure flags never change results.
 * d_best_dist receives npat uint8, d_best_count npat uint64, each entry written once.  Its
 * temporaries (two index lists of npat uint64 and the lists' lengths, for k >= 1) are
 * allocated stream-ordered; it reads no environment.  npat == 0 is CS_OK with nothing
 * touched; null outputs with npat > 0 are CS_ERR_INVALID. */
cs_status cs_fm_best_mismatch_device(const cs_fm_index* h, const uint8_t* d_pats,
                                     const uint64_t* d_offs, uint64_t fixed_m, uint64_t npat,
                                     uint32_t k, uint8_t* d_best_dist, uint64_t* d_best_count,
                                     uint32_t flags, void* stream);

/* Host batch (pattern q = pats[offs[q] .. offs[q + 1]), offsets non-decreasing, else
 * CS_ERR_INVALID), staged through HBM in one copy; out_dist receives npat uint8, out_count
 * npat uint64.  Synchronises before returning. */
cs_status cs_fm_best_mismatch_batch(const cs_fm_index* h, const uint8_t* pats,
                                    const uint64_t* offs, uint64_t npat, uint32_t k,
                                    uint8_t* out_dist, uint64_t* out_count, void* stream);

/* One pattern, host: *out_dist and *out_count; null outputs are CS_ERR_INVALID. */
cs_status cs_fm_best_mismatch(const cs_fm_index* h, const uint8_t* pattern, uint64_t m,
                              uint32_t k, uint8_t* out_dist, uint64_t* out_count);

#ifdef __cplusplus
}
#endif
#endif /* CS_FMINDEX_APPROX_BEST_H */

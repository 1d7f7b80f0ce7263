/*
 * cs_fmindex_approx_best_locate.h — best-stratum locate: the positions of a pattern at its
 * smallest mismatch distance, and nothing else.  What a read mapper asks after
 * cs_fmindex_approx_best.h's "how close?": "where are the best hits?".
 *
 * For a pattern P, a bound k <= CS_MM_MAX and the pairs (pos, d) of
 * cs_fmindex_approx_locate.h:
 *
 *     best_dist[q] = cs_fm_best_mismatch's value: the smallest d <= k with hist[d] > 0
 *                    (uint8; CS_MM_NONE when none)
 *     positions    = the pos of cs_fm_locate_mismatch's pairs with d == best_dist[q]
 *
 * in CSR form: out_offs[npat + 1] and out_pos[total].  There is no distance per position: the
 * distance is per pattern.  For m > 0 a pattern's size, out_offs[q + 1] - out_offs[q], equals
 * cs_fm_best_mismatch's best_count.
 *
 * Every quirk is inherited: m = 0 gives best_dist 0 and no positions (as the best-stratum call
 * and the locate calls each do); n = 0 gives CS_MM_NONE and no positions; a symbol absent from
 * the text never counts; d > m never resolves; k = 0 is the exact locate, with CS_MM_NONE
 * where it is empty; k > CS_MM_MAX is CS_ERR_INVALID.
 *
 * Order inside a pattern: the traversal's own — the order in which
 * cs_fm_locate_mismatch_device at the same k writes that pattern's pairs with
 * d == best_dist (the depth-d leaves of the depth-first search keep their relative order
 * whatever deeper frames do); one leaf's positions are contiguous and in row order.  With
 * k = 0 the output is exactly cs_fm_locate_device's.
 *
 * The search runs in rounds d = 0..k as cs_fm_best_mismatch_device's: round d searches, at
 * exactly d mismatches, the patterns with no hit below d.  Each pattern is searched twice at
 * its own distance (sizing, emitting) and once at every distance below it; no pattern pays for
 * a distance above its own.
 *
 * Capacity as in cs_fmindex_approx_locate.h: when total > cap the call returns
 * CS_ERR_CAPACITY with *total, the offsets and best_dist written, positions untouched;
 * cap = 0 with a null position buffer is the sizing call — which is therefore also a
 * best-stratum call, its counts being the offsets' differences.
 */
#ifndef CS_FMINDEX_APPROX_BEST_LOCATE_H
#define CS_FMINDEX_APPROX_BEST_LOCATE_H

#include <stdint.h>

#include "cs_fmindex.h"
#include "cs_fmindex_approx.h"
#include "cs_fmindex_approx_best.h"
#include "cs_fmindex_approx_locate.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device batch.  Pattern layout and null rules exactly as cs_fm_best_mismatch_device's and
 * cs_fm_locate_mismatch_device's: CSR offsets d_offs[npat + 1] into d_pats (unchecked), or
 * d_offs == NULL for npat patterns of fixed_m bytes back to back; d_pats may be NULL when
 * every pattern is empty.  d_best_dist receives npat uint8, d_out_offs npat + 1 uint64,
 * d_out_pos *total uint64 (cap: its capacity in entries).  npat == 0 writes d_out_offs[0] = 0
 * and *total = 0 and touches nothing else.  flags: the CS_Q_* structure flags (they never
 * change results); CS_Q_NO_FULL_SA and CS_Q_NO_WALK_LINES select the position phase as in
 * cs_fm_locate_mismatch_device.  An LF overrun is CS_ERR_LF_OVERRUN, as the exact locate
 * reports it, and the handle stays usable.  Synchronises stream once for the read-back of the
 * totals between sizing and emitting (and, as every checked locate, for the overrun word at
 * the end); allocates its temporaries stream-ordered and reads no environment. */
cs_status cs_fm_locate_best_mismatch_device(const cs_fm_index* h, const uint8_t* d_pats,
    const uint64_t* d_offs, uint64_t fixed_m, uint64_t npat, uint32_t k,
    uint8_t* d_best_dist, uint64_t* d_out_offs, uint64_t* d_out_pos, uint64_t cap,
    uint64_t* total, uint32_t flags, void* stream);

/* Host batch (pattern q = pats[offs[q] .. offs[q + 1]), offsets non-decreasing, else
 * CS_ERR_INVALID), staged through HBM once; out_dist receives npat uint8, out_offs npat + 1
 * uint64.  With cap too small it returns CS_ERR_CAPACITY after the sizing step (out_dist,
 * out_offs and *total written), without running the position phase. */
cs_status cs_fm_locate_best_mismatch_batch(const cs_fm_index* h, const uint8_t* pats,
    const uint64_t* offs, uint64_t npat, uint32_t k, uint8_t* out_dist, uint64_t* out_offs,
    uint64_t* out_pos, uint64_t cap, uint64_t* total, void* stream);

/* One pattern, host: *out_dist and *nout positions in out_pos. */
cs_status cs_fm_locate_best_mismatch(const cs_fm_index* h, const uint8_t* pattern, uint64_t m,
    uint32_t k, uint8_t* out_dist, uint64_t* out_pos, uint64_t cap, uint64_t* nout);

#ifdef __cplusplus
}
#endif
#endif /* CS_FMINDEX_APPROX_BEST_LOCATE_H */

/*
 * cs_fmindex_approx_locate.h — approximate locate: positions within k mismatches, with their
 * distances.  The companion of cs_fmindex_approx.h's count.
 *
 * For a pattern P of length m and a bound k <= CS_MM_MAX the result is the set of pairs
 * (pos, d), d <= k, where pos is a position the exact locate of include/cs_fmindex.h (the
 * reference's FMIndex::locate, src/api/fm_index.cpp:107-157, with no limit) reports for some
 * byte string S with |S| = m and Hamming(S, P) = d.  Its quirks come along: a cyclic BWT with
 * positions taken % n, a symbol absent from the text contributes nothing, the terminator and
 * rare symbols are substitutes like any other, m = 0 gives no positions (fm_index.cpp:109 —
 * although the count's hist[0] is n there), n = 0 gives none, there is no cap on m.  Wherever
 * the exact locate succeeds a position occurs at most once per pattern (it spells one S).
 *
 * A batch result is in CSR form: out_offs[npat + 1] (the exclusive scan of the per-pattern
 * totals; for m > 0 a pattern's total is the sum of its cs_fm_count_mismatch histogram row),
 * out_pos[total] and out_dist[total].
 *
 * Order inside a pattern: the search's own, a depth-first traversal whose leaves are the
 * neighbours S that occur — at each pattern position, from the last to the first, every
 * substitute in ascending byte order (each one's subtree first), then the pattern's own
 * character.  The positions of one leaf (one S) are contiguous and in row order, as the exact
 * locate reports them; with k = 0 the output is exactly cs_fm_locate_device's.  Beyond that the
 * order is unspecified: sort by (pos) or (dist, pos) if you need one.
 *
 * There is no per-pattern limit ("the first L in search order" would mean nothing).  Size the
 * output from the count's histogram or from a first call: when total > cap the call returns
 * CS_ERR_CAPACITY with *total set and the offsets written, positions and distances untouched;
 * cap = 0 with null position and distance buffers is the sizing call.
 */
#ifndef CS_FMINDEX_APPROX_LOCATE_H
#define CS_FMINDEX_APPROX_LOCATE_H

#include <stdint.h>

#include "cs_fmindex.h"
#include "cs_fmindex_approx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device batch.  Pattern layout exactly as cs_fm_count_mismatch_device's: CSR offsets
 * d_offs[npat + 1] into d_pats (unchecked), or d_offs == NULL for npat patterns of fixed_m
 * bytes back to back; d_pats may be NULL when every pattern is empty.  d_out_offs receives
 * npat + 1 uint64, d_out_pos and d_out_dist *total entries each (cap: their capacity in
 * entries).  flags: the CS_Q_* structure flags with their usual meaning (they never change
 * results); CS_Q_NO_FULL_SA and CS_Q_NO_WALK_LINES select the position phase as in
 * cs_fm_locate_walk_device.  An LF overrun is CS_ERR_LF_OVERRUN, as the exact locate reports
 * it.  Synchronises stream (the total is read back between the two passes of the search);
 * allocates its temporaries stream-ordered and reads no environment. */
cs_status cs_fm_locate_mismatch_device(const cs_fm_index* h, const uint8_t* d_pats,
                                       const uint64_t* d_offs, uint64_t fixed_m, uint64_t npat,
                                       uint32_t k, uint64_t* d_out_offs, uint64_t* d_out_pos,
                                       uint8_t* d_out_dist, uint64_t cap, uint64_t* total,
                                       uint32_t flags, void* stream);

/* Host batch (pattern q = pats[offs[q] .. offs[q + 1]), offsets non-decreasing, else
 * CS_ERR_INVALID), staged through HBM once.  With cap too small it returns CS_ERR_CAPACITY
 * after the sizing step, without running the position phase. */
cs_status cs_fm_locate_mismatch_batch(const cs_fm_index* h, const uint8_t* pats,
                                      const uint64_t* offs, uint64_t npat, uint32_t k,
                                      uint64_t* out_offs, uint64_t* out_pos, uint8_t* out_dist,
                                      uint64_t cap, uint64_t* total, void* stream);

/* One pattern, host: *nout pairs (out_pos[i], out_dist[i]). */
cs_status cs_fm_locate_mismatch(const cs_fm_index* h, const uint8_t* pattern, uint64_t m,
                                uint32_t k, uint64_t* out_pos, uint8_t* out_dist, uint64_t cap,
                                uint64_t* nout);

#ifdef __cplusplus
}
#endif
#endif /* CS_FMINDEX_APPROX_LOCATE_H */

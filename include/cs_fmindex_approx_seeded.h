/*
 * cs_fmindex_approx_seeded.h — seeded approximate locate: positions within k mismatches, with
 * their distances, by pigeonhole seeds verified against the text.  A second way to the pair set
 * of cs_fmindex_approx_locate.h, for the patterns its backtracking search cannot reach: long
 * ones and bounds past CS_MM_MAX.
 *
 * For a pattern P of length m >= 1 and a bound k <= CS_SEED_MAX_K the result is the set of pairs
 * (i, d), d = Hamming(P, t[(i + j) mod n], j < m) <= k, over every start i in [0, n), each pair
 * exactly once per pattern; m = 0 gives no pairs.  That is cs_fmindex_approx_locate.h's result
 * wherever the BWT rows are the text's rotations — a unique smallest last symbol, the handle's
 * lf_exact — and only such handles are served, and only those that keep the byte text in HBM
 * (cs_fm_info.text_in_hbm): anything else is CS_ERR_UNSUPPORTED, the message naming what is
 * missing.  k > CS_SEED_MAX_K is CS_ERR_INVALID, and so is a non-empty pattern with m <= k (every
 * start would qualify and a piece would be empty), the message naming the first such pattern.
 * All of it is checked before any output is touched.
 *
 * How: the pattern is cut into k + 1 pieces, piece p = P[a_p, a_{p+1}) with
 * a_p = floor(p * m / (k + 1)), p = 0..k.  A window within k substitutions of P holds at least
 * one piece unchanged, so the pieces are located exactly (the two-phase exact locate of
 * cs_fmindex.h, on any index layout) and every hit of piece p at text position x proposes the
 * alignment s = (x - a_p) mod n, which is compared with the text.  An alignment is emitted by
 * the first piece that matches it exactly: a candidate from piece p is dropped when some piece
 * p' < p has no mismatch at s, so no sort and no duplicate removal is needed.
 *
 * Order inside a pattern: pieces ascending, and inside a piece that piece's exact-locate row
 * order.  With k = 0 the output is exactly cs_fm_locate_device's with limit >= n.
 *
 * Cost: k + 1 exact searches per pattern, one position and one window comparison of at most m
 * bytes per candidate, C = the sum of the pieces' exact counts being the number of candidates
 * (*candidates).  On long patterns a piece has about one hit and the cost hardly depends on k;
 * on short patterns over a large text C is what the call costs (a 10-mer piece of a 20-mer at
 * k = 1 has n / 4^10 chance hits).  Temporaries, stream-ordered: about 17 bytes per candidate
 * and 32 bytes per piece.  When they cannot be allocated the call fails with CS_ERR_OOM and C
 * in the message; it never splits the batch on its own.
 *
 * A batch result is in CSR form as cs_fmindex_approx_locate.h's: out_offs[npat + 1],
 * out_pos[total], out_dist[total].  When total > cap the call returns CS_ERR_CAPACITY with
 * *total set and the offsets written, positions and distances untouched; cap = 0 with null
 * position and distance buffers is the sizing call.
 */
#ifndef CS_FMINDEX_APPROX_SEEDED_H
#define CS_FMINDEX_APPROX_SEEDED_H

#include <stdint.h>

#include "cs_fmindex.h"

#define CS_SEED_MAX_K 15u

#ifdef __cplusplus
extern "C" {
#endif

/* Device batch.  Pattern layout, flags and stream rules exactly as
 * cs_fm_locate_mismatch_device's: CSR offsets d_offs[npat + 1] into d_pats (unchecked), or
 * d_offs == NULL for npat patterns of fixed_m bytes back to back; d_pats may be NULL when every
 * pattern is empty and may have any alignment.  d_out_offs receives npat + 1 uint64, d_out_pos
 * and d_out_dist *total entries each (cap: their capacity in entries).  candidates: NULL, or
 * receives C.  flags: the CS_Q_* structure flags go to the piece search and the position phase
 * (they never change results).  A length m <= k is found on the host for fixed_m and by the
 * piece kernel for CSR offsets.  An LF overrun of the position phase is CS_ERR_LF_OVERRUN.
 * Synchronises stream twice: after the piece search (C is read back) and after the scan (the
 * total); reads no environment. */
cs_status cs_fm_locate_mismatch_seeded_device(const cs_fm_index* h, const uint8_t* d_pats,
                                              const uint64_t* d_offs, uint64_t fixed_m,
                                              uint64_t npat, uint32_t k, uint64_t* d_out_offs,
                                              uint64_t* d_out_pos, uint8_t* d_out_dist,
                                              uint64_t cap, uint64_t* total, uint64_t* candidates,
                                              uint32_t flags, void* stream);

/* Host batch (pattern q = pats[offs[q] .. offs[q + 1]), offsets non-decreasing, else
 * CS_ERR_INVALID), staged through HBM once. */
cs_status cs_fm_locate_mismatch_seeded_batch(const cs_fm_index* h, const uint8_t* pats,
                                             const uint64_t* offs, uint64_t npat, uint32_t k,
                                             uint64_t* out_offs, uint64_t* out_pos,
                                             uint8_t* out_dist, uint64_t cap, uint64_t* total,
                                             uint64_t* candidates, void* stream);

/* One pattern, host: *nout pairs (out_pos[i], out_dist[i]). */
cs_status cs_fm_locate_mismatch_seeded(const cs_fm_index* h, const uint8_t* pattern, uint64_t m,
                                       uint32_t k, uint64_t* out_pos, uint8_t* out_dist,
                                       uint64_t cap, uint64_t* nout);

#ifdef __cplusplus
}
#endif
#endif /* CS_FMINDEX_APPROX_SEEDED_H */

// fm_walk.hpp — the LF walk of FMIndex::locate (src/api/fm_index.cpp:125-153) over walk lines
// (fm_device.hpp WalkLine / WalkLineW), as device helpers: from a BWT row, follow LF until a
// marked row or a row the reference samples, then add the steps to that row's sample.  The
// rule is stated once here — the stop test (walk_stop_at / walk_stop), the single walk
// (walk_one) and the lockstep walk (walk_lockstep) — for phase 2 of locate (fm_walk.hip) and
// for the one-call locate and k_count_long's walk-verify forms (fm_query.hip).
#pragma once
#include "fm_search.hpp"

namespace fmx {
namespace {

// the walk lines of a kernel's kPos / kWalk parameter: 1 narrow (WalkLine), 2 wide (WalkLineW)
template <int kPos>
using WalkLineOf = std::conditional_t<kPos == 1, WalkLine, WalkLineW>;

// the rows the reference samples (row % stride == 0) and their index in the SSA, for the
// walk over the engine's own LF (k_walk); POW2: the stride is a power of two
template <bool POW2>
__device__ __forceinline__ bool is_sampled(const DevIndex& ix, uint64_t row) {
  if (POW2) return (row & ((1ull << ix.stride_shift) - 1)) == 0;
  return row % ix.stride == 0;
}

template <bool POW2>
__device__ __forceinline__ uint64_t sample_index(const DevIndex& ix, uint64_t row) {
  if (POW2) return row >> ix.stride_shift;
  return row / ix.stride;
}

// sample k of the marked rows
__device__ __forceinline__ uint64_t wssa_at(const DevIndex& ix, uint64_t k) {
  if (ix.wssa_eb == 5) {  // 40-bit entries (wide position samples): the two dwords holding them
    const uint64_t b = 5 * k;
    const uint32_t* d = static_cast<const uint32_t*>(ix.wssa) + (b >> 2);
    const uint64_t x = ((uint64_t)d[1] << 32) | d[0];
    return (x >> (8 * (b & 3))) & ((1ull << 40) - 1);
  }
  return ix.wssa_eb == 8 ? static_cast<const uint64_t*>(ix.wssa)[k] : static_cast<const uint32_t*>(ix.wssa)[k];
}

// LF(pos) from pos's walk line v (line q, offset o): C[c] + occ(c, pos) from the same
// line (OccE::lf), or for the quaternary matrix level 0 from the walk line and levels
// 1.. as QWM::lf.
template <class W, bool kQ>
__device__ __forceinline__ uint64_t walk_lf(const DevIndex& ix, const NodeTable& T,
                                            const typename W::Raw& v, uint64_t q, uint32_t o,
                                            uint64_t pos) {
  if (!kQ) {
    const uint32_t code = W::code(v, o);
    uint32_t c = T.occ_sym[code];
    uint64_t r = W::occ(v, code, q, o);
    if (code == 0 && T.exc_n) {
      const uint32_t e = exc_before(T, pos);
      if (e < T.exc_n && T.exc_row[e] == pos) {
        c = T.exc_sym[e];
        r = exc_rank(T, c, pos);
      } else {
        r -= e;
      }
    }
    return T.C[c] + r;
  }
  const uint32_t d0 = W::code(v, o);
  uint64_t p = T.qZ[0][d0] + W::occ(v, d0, q, o);
  uint32_t x = d0;
  const int L = (int)T.qlevels;
  for (int l = 1; l < L; ++l) {
    const int nid = qnode_id(l, x);
    const uint8_t f = T.flags[nid];
    uint32_t d;
    if (f & kPure) {
      d = (f >> 2) & 3u;
      p = T.qZ[l][d] + T.R[nid] + (p - T.S[nid]);
    } else {
      OccLine::Raw lv;
      const uint64_t lq = p >> 6;
      OccLine::load(QWM::level(ix, l), lq, lv);
      const uint32_t lo = (uint32_t)(p & 63);
      d = OccLine::code(lv, lo);
      p = T.qZ[l][d] + OccLine::base(lv, d, lq) + OccLine::prefix(lv, d, lo);
    }
    x = (x << 2) | d;
  }
  return T.C[T.qsym[x]] + (p - T.S8[x]);
}

// the constants an LF step of a walk reads from the node table, held in registers by a
// barrier-free kernel whose table is the global one (a walk step through the caches waits on
// two more dependent loads: round 5, C5's one-call search 1.56 -> 1.70 ms that way)
struct WalkK {
  uint64_t C[4];     // C[] of each occurrence code's symbol
  uint32_t nexc;     // rare rows
  uint64_t exc_row0; // the rare row when there is one (C5's terminator), and C[] of its symbol
  uint64_t exc_c0;
};
__device__ __forceinline__ WalkK walk_consts(const NodeTable& T) {
  WalkK k;
#pragma unroll
  for (int c = 0; c < 4; ++c) k.C[c] = T.C[T.occ_sym[c]];
  k.nexc = T.exc_n;
  k.exc_row0 = k.nexc ? T.exc_row[0] : 0;
  k.exc_c0 = k.nexc ? T.C[T.exc_sym[0]] : 0;
  return k;
}

// walk_lf over the occurrence-line walk lines with the step's constants in registers (K);
// more than one rare row takes the table (through the caches) as walk_lf does
template <class W>
__device__ __forceinline__ uint64_t walk_lf_k(const NodeTable& T, const WalkK& K, const typename W::Raw& v,
                                              uint64_t q, uint32_t o, uint64_t pos) {
  const uint32_t code = W::code(v, o);
  uint64_t r = W::occ(v, code, q, o);
  const uint64_t cc = code == 0 ? K.C[0] : code == 1 ? K.C[1] : code == 2 ? K.C[2] : K.C[3];
  if (code == 0 && K.nexc) {
    if (K.nexc == 1) {
      if (pos == K.exc_row0) return K.exc_c0;  // the rare row: no earlier row holds its symbol
      r -= K.exc_row0 < pos ? 1u : 0u;
    } else {
      const uint32_t e = exc_before(T, pos);
      if (e < T.exc_n && T.exc_row[e] == pos) {
        const uint32_t c = T.exc_sym[e];
        return T.C[c] + exc_rank(T, c, pos);
      }
      r -= e;
    }
  }
  return cc + r;
}

// ---- where a walk stops ----
// A walk may stop at a marked row or at a row the reference samples (row % stride == 0,
// SSA): both give SA[start] = sample + steps (mod n, fm_index.cpp:147-153), and the first of
// the two comes sooner (mean 11 steps at stride 32 instead of 15.5).
// The test in two halves, for a walk that reads the line in one loop iteration and the
// sample in the next (k_walk_lines): walk_stop_at — is row `pos` (walk line v, offset o) a
// stop row, and which sample holds its position — then walk_sample, the one load, and
// walk_start.  walk_stop is the two together.
struct WalkStop {
  uint64_t sidx;  // the sample's index
  bool from_ssa;  // in the reference's row samples (ssa), else in the marks' samples (wssa)
};
template <class W>
__device__ __forceinline__ bool walk_stop_at(const DevIndex& ix, const typename W::Raw& v, uint32_t o,
                                             uint64_t pos, WalkStop& stop) {
  const uint64_t row_mask = ix.stride_shift != 0xFFFFFFFFu ? (1ull << ix.stride_shift) - 1 : 0;
  const bool mk = W::mark(v, o);
  const bool rs = row_mask ? (pos & row_mask) == 0 : pos % ix.stride == 0;
  if (!(mk || rs)) return false;
  stop.from_ssa = !mk;
  stop.sidx = mk ? W::mark_rank(v, o) : (row_mask ? pos >> ix.stride_shift : pos / ix.stride);
  return true;
}
__device__ __forceinline__ uint64_t walk_sample(const DevIndex& ix, const WalkStop& stop) {
  return stop.from_ssa ? ssa_at(ix, stop.sidx) : wssa_at(ix, stop.sidx);
}
// the position of the row a walk started from: `steps` LF steps before the sample's
__device__ __forceinline__ uint64_t walk_start(uint64_t sample, uint64_t steps, uint64_t n) {
  const uint64_t s = sample + steps;
  return s >= n ? s - n : s;
}
// true: row `pos`, reached after `steps` LF steps, is a stop row, and pos is now the
// position of the row the walk started from
template <class W>
__device__ __forceinline__ bool walk_stop(const DevIndex& ix, const typename W::Raw& v, uint32_t o,
                                          uint64_t& pos, uint64_t steps) {
  WalkStop stop;
  if (!walk_stop_at<W>(ix, v, o, pos, stop)) return false;
  pos = walk_start(walk_sample(ix, stop), steps, ix.n);
  return true;
}

// ---- the single walk ----
// The text position of BWT row `pos`: by LF to the first stop row, one walk line per step.
// steps = the LF steps taken; n on overrun (fm_index.cpp:130, :136-138: no stop row within n
// steps; the result is then 0).  An lf_exact index with text-position marks ends every walk
// within pstride - 1 steps.  kQ: the walk lines of a quaternary matrix.
template <class W, bool kQ>
__device__ __forceinline__ uint64_t walk_one(const DevIndex& ix, const NodeTable& T, uint64_t pos,
                                             uint64_t& steps) {
  const uint64_t n = ix.n;
  for (steps = 0; steps < n; ++steps) {
    uint64_t q;
    uint32_t o;
    typename W::Raw v;
    W::locate(pos, q, o);
    W::load(ix.walk, q, v);
    if (walk_stop<W>(ix, v, o, pos, steps)) return pos;
    pos = walk_lf<W, kQ>(ix, T, v, q, o, pos);
  }
  return 0;
}

template <class W>
__device__ __forceinline__ uint64_t walk_position(const DevIndex& ix, const NodeTable& T, uint64_t row) {
  uint64_t steps;
  return walk_one<W, false>(ix, T, row, steps);
}

// One walk of phase 2: writes out[j] = the text position of `row` minus adj (mod n), or the
// LF steps when steps_only (the measurement twin: bench.py's walk bytes); an overrun records
// j in err.
template <class W, bool kQ>
__device__ __forceinline__ void walk_short_one(const DevIndex& ix, const NodeTable& T, uint64_t row,
                                               uint64_t adj, uint64_t j, uint64_t* __restrict__ out,
                                               unsigned long long* __restrict__ err,
                                               uint32_t steps_only) {
  const uint64_t n = ix.n;
  uint64_t steps;
  const uint64_t s = walk_one<W, kQ>(ix, T, row, steps);
  if (steps >= n) {
    atomicMin(err, (unsigned long long)j);
    return;
  }
  st_out(out + j, steps_only ? steps : pos_back(s, adj, n));
}

// ---- the lockstep walk ----
// U rows of a lane walked together, their line reads in flight together: pos[j] becomes the
// text position of row pos[j] where act[j] (cleared as the walks end).  lf(v, q, o, pos) is
// the LF step from a row's walk line: walk_lf over the block's table (walk_positions) or
// walk_lf_k over constants in registers (walk_positions_k).
template <class W, int U, class LF>
__device__ __forceinline__ void walk_lockstep(const DevIndex& ix, uint64_t* pos, bool* act, LF lf) {
  const uint64_t n = ix.n;
  uint64_t steps[U];
#pragma unroll
  for (int j = 0; j < U; ++j) steps[j] = 0;
  for (uint64_t it = 0; it < n; ++it) {
    bool any = false;
#pragma unroll
    for (int j = 0; j < U; ++j) any |= act[j];
    if (!any) return;
    uint64_t q[U];
    uint32_t o[U];
    typename W::Raw v[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {  // the lines of every active walk first
      q[j] = 0, o[j] = 0;
      if (act[j]) {
        W::locate(pos[j], q[j], o[j]);
        W::load(ix.walk, q[j], v[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < U; ++j) {
      if (!act[j]) continue;
      if (walk_stop<W>(ix, v[j], o[j], pos[j], steps[j])) {
        act[j] = false;
      } else {
        pos[j] = lf(v[j], q[j], o[j], pos[j]);
        ++steps[j];
      }
    }
  }
}

template <class W, int U>
__device__ __forceinline__ void walk_positions(const DevIndex& ix, const NodeTable& T, uint64_t* pos,
                                               bool* act) {
  walk_lockstep<W, U>(ix, pos, act, [&](const typename W::Raw& v, uint64_t q, uint32_t o, uint64_t p) {
    return walk_lf<W, false>(ix, T, v, q, o, p);
  });
}

template <class W, int U>
__device__ __forceinline__ void walk_positions_k(const DevIndex& ix, const NodeTable& T, const WalkK& K,
                                                 uint64_t* pos, bool* act) {
  walk_lockstep<W, U>(ix, pos, act, [&](const typename W::Raw& v, uint64_t q, uint32_t o, uint64_t p) {
    return walk_lf_k<W>(T, K, v, q, o, p);
  });
}

}  // namespace
}  // namespace fmx

// fm_walk.hip — phase 2 of locate (cs_fm_locate_walk_device, FMIndex::locate's
// src/api/fm_index.cpp:125-157): the positions of every reported row of a batch, from the
// records and offsets phase 1 wrote (launch_locate_ranges, fm_query.hip; the mismatch locates
// hand their leaves: fm_mismatch.hip).  With the full suffix array one SA read per row
// (k_locate_sa); otherwise the LF walk of fm_walk.hpp — short walks over walk lines with
// text-position marks, straight from the records (k_walk_fused) or from an expanded rows
// buffer (k_expand_rows + k_walk_short) — or a persistent walk: each block owns a contiguous
// slice of rows, its lanes pull rows from an LDS counter and cycle fetch -> walk -> sample
// with one dependent load per loop iteration, over walk lines (k_walk_lines: one 32-B read
// per step gives the symbol, its occ and the sample mark; no separate BWT array is kept) or
// over the engine's own LF (k_walk).
#include "fm_walk.hpp"

namespace fmx {

// Phase 2 with the full suffix array, fused (no rows buffer): each pattern's rows come
// from its record (LocRows) and go straight through SA: SA[row] - k (mod n) for
// a window row k characters before the end, SA[row] otherwise.  A lane
// takes a pattern of at most kLocSmall rows (every context window: <= kLocSpanBits);
// wider plain ranges are listed for k_locate_sa_wide, a block per range.
// (These two kernels keep their external names.)
__global__ __launch_bounds__(kBlk) void k_locate_sa(const uint32_t* __restrict__ sa, uint64_t n,
                                                    const uint64_t* __restrict__ sp,
                                                    const uint64_t* __restrict__ offs, uint64_t npat,
                                                    uint64_t* __restrict__ out,
                                                    uint64_t* __restrict__ wide,
                                                    unsigned long long* __restrict__ nwide) {
  const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; q < npat; q += gs) {
    const uint64_t a = offs[q], c = offs[q + 1] - a, s = sp[q];
    if (!c) continue;
    LocRows rows = LocRows::of(s);
    if (s & kLocCtx) {  // scattered rows, read once
      const uint64_t adj = rows.adj;
      for (uint64_t j = 0; j < c; ++j) {
        const uint64_t p = load_sa(sa, rows.next());
        st_out(out + a + j, pos_back(p, adj, n));
      }
    } else if (c <= kLocSmall) {  // consecutive rows: the lane's reads share their sectors
      for (uint64_t j = 0; j < c; ++j) st_out(out + a + j, (uint64_t)sa[rows.next()]);
    } else {
      wide[atomicAdd(nwide, 1ull)] = q;
    }
  }
}

__global__ __launch_bounds__(kBlk) void k_locate_sa_wide(const uint32_t* __restrict__ sa,
                                                         const uint64_t* __restrict__ sp,
                                                         const uint64_t* __restrict__ offs,
                                                         uint64_t* __restrict__ out,
                                                         const uint64_t* __restrict__ wide,
                                                         const unsigned long long* __restrict__ nwide) {
  const uint64_t nw = *nwide;
  for (uint64_t e = blockIdx.x; e < nw; e += gridDim.x) {
    const uint64_t q = wide[e], a = offs[q], c = offs[q + 1] - a, s = sp[q];
    for (uint64_t j = threadIdx.x; j < c; j += blockDim.x) st_out(out + a + j, (uint64_t)sa[s + j]);
  }
}

namespace {

// The reported rows of pattern q in row order (fm_index.cpp:125), each tagged with its
// window's k (row | k << kWalkAdjShift; a plain range's rows untagged).
__global__ void k_expand_rows(const uint64_t* __restrict__ sp, const uint64_t* __restrict__ offs,
                              uint64_t npat, uint64_t* __restrict__ rows) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; q < npat; q += stride) {
    const uint64_t a = offs[q], b = offs[q + 1];
    LocRows it = LocRows::of_walk(sp[q]);
    const uint64_t tag = it.adj << kWalkAdjShift;
    for (uint64_t j = a; j < b; ++j) rows[j] = it.next() | tag;
  }
}

// Persistent LF walk (fm_index.cpp:125-153) over the engine's own LF, to the rows the
// reference samples: no walk lines, so only the skeleton is k_walk_lines'.  Block b owns
// rows [b*chunk, ...); lanes pull rows from an LDS counter and cycle FETCH -> WALK -> SAMPLE
// as in k_walk_lines below (the SSA read of a finishing lane does not add a round trip
// to its wave's LF step).
template <class E, bool POW2>
__global__ __launch_bounds__(kBlk) void k_walk(DevIndex ix, const uint64_t* __restrict__ rows,
                                               uint64_t total, uint64_t chunk,
                                               uint64_t* __restrict__ out,
                                               unsigned long long* __restrict__ err,
                                               uint32_t steps_only) {
  enum : uint32_t { kFetch = 0, kWalk = 1, kSample = 2, kDone = 3 };
  __shared__ NodeTable T;
  __shared__ unsigned long long next;
  const uint64_t a = blockIdx.x * chunk;
  const uint64_t end = (a + chunk < total) ? a + chunk : total;
  load_table(T, ix.table);
  if (threadIdx.x == 0) next = a;
  __syncthreads();
  if (a >= total) return;
  const uint64_t n = ix.n;
  uint64_t j = 0, pos = 0, steps = 0, adj = 0;
  uint32_t phase = kFetch;
  for (;;) {
    if (phase == kFetch) {
      j = atomicAdd(&next, 1ull);
      if (j >= end) phase = kDone;
    }
    if (!__any(phase != kDone)) break;
    uint64_t row = 0, smp = 0;
    if (phase == kFetch) row = rows[j];
    if (phase == kSample) smp = ssa_at(ix, sample_index<POW2>(ix, pos));
    if (phase == kFetch) {
      pos = row & kWalkRowMask;
      adj = row >> kWalkAdjShift;
      steps = 0;
      phase = kWalk;
    } else if (phase == kSample) {
      const uint64_t s = walk_start(smp, steps, n);  // :147-153
      st_out(out + j, steps_only ? steps : pos_back(s, adj, n));
      phase = kFetch;
    } else if (phase == kWalk) {
      // loop condition of fm_index.cpp:130: stop at a sampled row or after n steps
      if (is_sampled<POW2>(ix, pos) || steps >= n) {
        if (steps >= n) {
          atomicMin(err, (unsigned long long)j);  // fm_index.cpp:136-138
          phase = kFetch;
        } else {
          phase = kSample;
        }
      } else {
        pos = E::lf(ix, T, pos);
        ++steps;
      }
    }
  }
}

// Short walks (walk lines with text-position marks, lf_exact): every walk ends within
// pstride - 1 steps, so one lane per reported row — coalesced row reads, no work
// queue — and finished waves make room for new ones, as in the count kernels.
template <class W, bool kQ>
__global__ __launch_bounds__(kBlk) void k_walk_short(DevIndex ix, const uint64_t* __restrict__ rows,
                                                     uint64_t total, uint64_t* __restrict__ out,
                                                     unsigned long long* __restrict__ err,
                                                     uint32_t steps_only) {
  __shared__ NodeTable T;
  load_table(T, ix.table);
  __syncthreads();
  const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (j >= total) return;
  const uint64_t row = rows[j];
  walk_short_one<W, kQ>(ix, T, row & kWalkRowMask, row >> kWalkAdjShift, j, out, err, steps_only);
}

// Phase 2 over walk lines with text-position marks, fused with the records (no rows
// buffer, as k_locate_sa for the full SA): a lane takes a pattern's reported rows —
// a context window's matching rows (subtracting k) or a plain range of at most
// kLocSmall rows — and walks each; wider ranges are listed for k_walk_fused_wide.
template <class W, bool kQ>
__global__ __launch_bounds__(kBlk) void k_walk_fused(DevIndex ix, const uint64_t* __restrict__ sp,
                                                     const uint64_t* __restrict__ offs, uint64_t npat,
                                                     uint64_t* __restrict__ out,
                                                     uint64_t* __restrict__ wide,
                                                     unsigned long long* __restrict__ nwide,
                                                     unsigned long long* __restrict__ err,
                                                     uint32_t steps_only) {
  __shared__ NodeTable T;
  load_table(T, ix.table);
  __syncthreads();
  const uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (q >= npat) return;
  const uint64_t a = offs[q], c = offs[q + 1] - a, s = sp[q];
  if (!c) return;
  if ((s & kLocCtx) || c <= kLocSmall) {
    LocRows rows = LocRows::of_walk(s);
    for (uint64_t j = 0; j < c; ++j)
      walk_short_one<W, kQ>(ix, T, rows.next(), rows.adj, a + j, out, err, steps_only);
  } else {
    wide[atomicAdd(nwide, 1ull)] = q;
  }
}

// the listed wide ranges: a block per range, its threads over the rows
template <class W, bool kQ>
__global__ __launch_bounds__(kBlk) void k_walk_fused_wide(DevIndex ix, const uint64_t* __restrict__ sp,
                                                          const uint64_t* __restrict__ offs,
                                                          uint64_t* __restrict__ out,
                                                          const uint64_t* __restrict__ wide,
                                                          const unsigned long long* __restrict__ nwide,
                                                          unsigned long long* __restrict__ err,
                                                          uint32_t steps_only) {
  __shared__ NodeTable T;
  load_table(T, ix.table);
  __syncthreads();
  const uint64_t nw = *nwide;
  for (uint64_t e = blockIdx.x; e < nw; e += gridDim.x) {
    const uint64_t q = wide[e], a = offs[q], c = offs[q + 1] - a, s = sp[q];
    for (uint64_t j = threadIdx.x; j < c; j += blockDim.x)
      walk_short_one<W, kQ>(ix, T, s + j, 0, a + j, out, err, steps_only);
  }
}

// The persistent walk over walk lines: one line per step gives the mark, the sample index
// and LF.
template <class W, bool kQ>
__global__ __launch_bounds__(kBlk) void k_walk_lines(DevIndex ix, const uint64_t* __restrict__ rows,
                                                     uint64_t total, uint64_t chunk,
                                                     uint64_t* __restrict__ out,
                                                     unsigned long long* __restrict__ err,
                                                     uint32_t steps_only) {
  // Each lane cycles FETCH (row from the block's slice) -> WALK (one line per LF
  // step) -> SAMPLE (the stop row's sample, with the next row's index) -> WALK ...
  // Every loop iteration issues at most one dependent load per lane and kind,
  // whatever its phase, so a wave waits one memory round trip per iteration even
  // when some of its lanes are starting or finishing a walk: the stop test
  // (walk_stop_at) in one iteration, its sample's load (walk_sample) in the next.
  enum : uint32_t { kFetch = 0, kWalk = 1, kSample = 2, kDone = 3 };
  __shared__ NodeTable T;
  __shared__ unsigned long long next;
  const uint64_t a = blockIdx.x * chunk;
  const uint64_t end = (a + chunk < total) ? a + chunk : total;
  load_table(T, ix.table);
  if (threadIdx.x == 0) next = a;
  __syncthreads();
  if (a >= total) return;
  const uint64_t n = ix.n;
  uint64_t j = 0, pos = 0, steps = 0, adj = 0;
  uint32_t phase = kFetch;
  WalkStop stop{0, false};
  for (;;) {
    if (phase == kFetch) {
      j = atomicAdd(&next, 1ull);
      if (j >= end) phase = kDone;
    }
    if (!__any(phase != kDone)) break;
    // ---- issue this iteration's load ----
    uint64_t row = 0, smp = 0, q = 0;
    uint32_t o = 0;
    typename W::Raw v;
    if (phase == kFetch) row = rows[j];
    if (phase == kWalk) {
      W::locate(pos, q, o);
      W::load(ix.walk, q, v);
    }
    uint64_t jn = 0;
    if (phase == kSample) {
      smp = walk_sample(ix, stop);
      // the next row's index travels with the sample: a walk of s steps costs s + 1
      // round trips instead of s + 2 (walks average ~3 steps at pstride 8)
      jn = atomicAdd(&next, 1ull);
      if (jn < end) row = rows[jn];
    }
    // ---- consume ----
    if (phase == kFetch) {
      pos = row & kWalkRowMask;
      adj = row >> kWalkAdjShift;
      steps = 0;
      phase = kWalk;
    } else if (phase == kWalk) {
      if (steps >= n) {  // fm_index.cpp:130 loop condition; :136-138, checked first
        atomicMin(err, (unsigned long long)j);
        phase = kFetch;
      } else if (walk_stop_at<W>(ix, v, o, pos, stop)) {
        phase = kSample;
      } else {
        pos = walk_lf<W, kQ>(ix, T, v, q, o, pos);
        ++steps;
      }
    } else if (phase == kSample) {
      const uint64_t s = walk_start(smp, steps, n);  // :147-153
      st_out(out + j, steps_only ? steps : pos_back(s, adj, n));
      if (jn < end) {
        j = jn;
        pos = row & kWalkRowMask;
        adj = row >> kWalkAdjShift;
        steps = 0;
        phase = kWalk;
      } else {
        phase = kDone;
      }
    }
  }
}

}  // namespace

cs_status launch_locate_walk(const cs_fm_index* h, const uint64_t* d_sp,
                             const uint64_t* d_out_offs, uint64_t npat, uint64_t total,
                             uint64_t* d_out_pos, hipStream_t st, unsigned long long* err_word,
                             uint32_t flags, uint32_t steps_only) {
  if (!total) return CS_OK;
  flags = call_flags(h, flags);
  if (h->d_sa && h->lf_exact && !(flags & CS_Q_NO_FULL_SA)) {  // full suffix array: one read per position
    if (steps_only) {  // no LF steps: one SA read per position
      FMX_HIP(hipMemsetAsync(d_out_pos, 0, total * 8, st));
      return CS_OK;
    }
    StreamBuf wide;
    FMX_HIP(wide.alloc((total / (kLocSmall + 1) + 1) * 8 + 8, st));
    unsigned long long* nwide = wide.as<unsigned long long>();
    FMX_HIP(hipMemsetAsync(nwide, 0, 8, st));
    const uint32_t* sa = static_cast<const uint32_t*>(h->d_sa);
    k_locate_sa<<<grid_for(npat, kBlk, 0xFFFFFFFFu), kBlk, 0, st>>>(
        sa, h->n, d_sp, d_out_offs, npat, d_out_pos, wide.as<uint64_t>() + 1, nwide);
    FMX_HIP(hipGetLastError());
    k_locate_sa_wide<<<1024, kBlk, 0, st>>>(sa, d_sp, d_out_offs, d_out_pos,
                                             wide.as<uint64_t>() + 1, nwide);
    FMX_HIP(hipGetLastError());
    return CS_OK;
  }
  int dev = 0, ncu = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
  const uint64_t max_blocks = (uint64_t)ncu * 8;  // 8 x 256 threads = full CU
  uint64_t chunk = (total + max_blocks - 1) / max_blocks;
  if (chunk < 64) chunk = 64;
  const unsigned blocks = (unsigned)((total + chunk - 1) / chunk);
  const DevIndex ix = query_dev(h, flags);
  unsigned long long* err =
      err_word ? err_word : reinterpret_cast<unsigned long long*>(h->d_err);
  // short_walk: walk lines with text-position marks, a short walk per position; unless
  // CS_QT_WALK_PERSISTENT (CS_FM_WALK_PERSISTENT=1): the persistent walk over a rows buffer
  const bool short_walk = ix.walk && h->walk_marks == 2 && !(flags & CS_QT_WALK_PERSISTENT);
  // fused: the short walks straight from the records (no rows buffer); unless CS_QT_WALK_ROWS
  // (CS_FM_WALK_ROWS=1): from an expanded rows buffer (k_expand_rows + k_walk_short)
  const bool fused = short_walk && !(flags & CS_QT_WALK_ROWS);
  // qwm: the walk lines are a quaternary matrix's (kQ); pow2: the sample stride is a power
  // of two (POW2; the persistent walk over the engine, an index without walk lines)
  const bool qwm = h->line_fmt == kFmtQwm;
  const bool pow2 = ix.stride_shift != 0xFFFFFFFFu;
  if (fused) {
    StreamBuf wide;
    FMX_HIP(wide.alloc((total / (kLocSmall + 1) + 1) * 8 + 8, st));
    unsigned long long* nwide = wide.as<unsigned long long>();
    FMX_HIP(hipMemsetAsync(nwide, 0, 8, st));
    uint64_t* wl = wide.as<uint64_t>() + 1;
    const unsigned g = grid_for(npat, kBlk, 0xFFFFFFFFu);
    with_walk_line(h->wide, [&](auto line) {
      with_bool(qwm, [&](auto kQ) {
        using W = typename decltype(line)::type;
        k_walk_fused<W, kQ><<<g, kBlk, 0, st>>>(ix, d_sp, d_out_offs, npat, d_out_pos, wl, nwide, err, steps_only);
        k_walk_fused_wide<W, kQ><<<1024, kBlk, 0, st>>>(ix, d_sp, d_out_offs, d_out_pos, wl, nwide, err, steps_only);
      });
    });
    FMX_HIP(hipGetLastError());
    return CS_OK;
  }
  StreamBuf rows;
  FMX_HIP(rows.alloc(total * 8, st));
  k_expand_rows<<<grid_for(npat, kBlk, 65536), kBlk, 0, st>>>(d_sp, d_out_offs, npat,
                                                              rows.as<uint64_t>());
  FMX_HIP(hipGetLastError());
  const uint64_t* r = rows.as<uint64_t>();
  if (ix.walk) {  // over walk lines: the short walks, or the persistent walk
    with_walk_line(h->wide, [&](auto line) {
      with_bool(qwm, [&](auto kQ) {
        using W = typename decltype(line)::type;
        if (short_walk)
          k_walk_short<W, kQ><<<grid_for(total, kBlk, 0xFFFFFFFFu), kBlk, 0, st>>>(ix, r, total, d_out_pos, err, steps_only);
        else
          k_walk_lines<W, kQ><<<blocks, kBlk, 0, st>>>(ix, r, total, chunk, d_out_pos, err, steps_only);
      });
    });
  } else {  // the persistent walk over the engine's own LF
    with_engine(h->line_fmt, [&](auto engine) {
      with_bool(pow2, [&](auto POW2) {
        using E = typename decltype(engine)::type;
        k_walk<E, POW2><<<blocks, kBlk, 0, st>>>(ix, r, total, chunk, d_out_pos, err, steps_only);
      });
    });
  }
  FMX_HIP(hipGetLastError());
  return CS_OK;  // rows are freed in stream order after the walk
}

cs_status check_locate_error(const cs_fm_index* h, unsigned long long* err, hipStream_t st) {
  if (!err) err = reinterpret_cast<unsigned long long*>(h->d_err);
  uint64_t bad = ~0ull;
  FMX_HIP(hipMemcpyAsync(&bad, err, 8, hipMemcpyDeviceToHost, st));
  FMX_HIP(hipStreamSynchronize(st));
  if (bad == ~0ull) return CS_OK;
  FMX_HIP(hipMemsetAsync(err, 0xFF, 8, st));
  FMX_HIP(hipStreamSynchronize(st));
  set_error("locate: LF walk exceeded text length");  // fm_index.cpp:137
  return CS_ERR_LF_OVERRUN;
}

}  // namespace fmx

// fm_mismatch.hip — search within k <= CS_MM_MAX mismatches: the per-distance count
// (cs_fmindex_approx.h), the best stratum (cs_fmindex_approx_best.h) and the two locates
// (cs_fmindex_approx_locate.h, cs_fmindex_approx_best_locate.h).  The depth-first searches of
// fm_search.hpp (mm_frame for the histograms, mm_leaves for the leaves) under four kernels, one
// pattern per lane, templates over the rank engine as the kernels of fm_query.hip; the helpers
// below are what the four share.  The
// positions of the locates come from the exact locate's walk (launch_locate_walk, fm_walk.hip)
// with the search's leaves as its patterns.
#include "fm_search.hpp"

namespace fmx {
namespace {

// The block's staging: the node table in LDS, then (kSyms) the substitute alphabet.  Every
// thread of the block calls it: it holds barriers.
template <bool kSyms>
__device__ __forceinline__ void mm_stage(NodeTable& T, SymList& L, const DevIndex& ix) {
  load_table(T, ix.table);
  __syncthreads();
  if constexpr (kSyms) list_symbols(L, T);
}

// Pattern q of the batch (offs == nullptr: patterns of one length fixed_m at stride fixed_m).
// Its bytes are read by index from global memory (they stay in the caches; no length cap).
// `search`: neither the pattern nor the text is empty; else fm_index.cpp:80-81 answer without
// a search — the empty pattern counts n and has no position (:109), an empty text holds nothing.
struct MmPat {
  const uint8_t* b;
  uint64_t m;
  bool search;
};
__device__ __forceinline__ MmPat mm_pattern(const DevIndex& ix, const uint8_t* pats,
                                            const uint64_t* offs, uint64_t fixed_m, uint64_t q) {
  const uint64_t o0 = offs ? offs[q] : q * fixed_m, m = offs ? offs[q + 1] - o0 : fixed_m;
  return MmPat{pats + o0, m, m != 0 && ix.n != 0};
}
// the exact count of a pattern that needs no search
__device__ __forceinline__ uint64_t mm_unsearched(const DevIndex& ix, const MmPat& p) {
  return p.m == 0 ? ix.n : 0;
}

// The work list of round K of a best-stratum search: round 0 runs over every pattern, round
// K >= 1 over the pending list of *len_in entries.  The grid is sized for npat (the host never
// reads a length); false: the block's first entry is at or past the list's length, and the
// block returns before it stages anything — a block-uniform test ahead of every barrier.
template <int K>
__device__ __forceinline__ bool mm_round_block(uint64_t npat, const unsigned long long* len_in,
                                               uint64_t& nlist) {
  nlist = npat;
  if constexpr (K > 0) {
    nlist = *len_in;
    return blockIdx.x * (uint64_t)blockDim.x < nlist;
  }
  return true;
}

// The sink of one pattern for a pass of a locate.  Sizing counts from zero and writes nothing.
// Emitting starts from the pattern's first leaf and output offset (cnt_leaf / cnt_occ hold the
// exclusive scans now) and never writes at or past the pattern's leaf end, whatever the second
// traversal does (LeafSink::leaf).
template <bool kEmit>
__device__ __forceinline__ LeafSink leaf_sink(uint64_t q, const uint64_t* cnt_leaf,
                                              const uint64_t* cnt_occ, uint64_t* leaf_sp,
                                              uint64_t* leaf_off, uint8_t* leaf_dist) {
  LeafSink sink;
  sink.nleaf = kEmit ? cnt_leaf[q] : 0;
  sink.nocc = kEmit ? cnt_occ[q] : 0;
  sink.end = kEmit ? cnt_leaf[q + 1] : 0;
  sink.leaf_sp = kEmit ? leaf_sp : nullptr;
  sink.leaf_off = leaf_off;
  sink.leaf_dist = leaf_dist;
  return sink;
}

// The histogram of a pattern that needs a search, added into h: h[d] += the summed exact counts
// of the strings at distance d, by the depth-first search of mm_frame (fm_search.hpp) from
// the pattern with no substitution yet (an unused SubPat slot has pos = ~0).
template <class E, int K>
__device__ __forceinline__ void mm_hist(const DevIndex& ix, const NodeTable& T, const SymList& L,
                                        const MmPat& p, uint64_t (&h)[K + 1]) {
  SubPat<K> S;
  S.b = p.b;
#pragma unroll
  for (int t = 0; t < K; ++t) S.pos[t] = ~0ull, S.sym[t] = 0;
  mm_frame<E, 0, K>(ix, T, L, S, p.m, p.m, 0, ix.n, h);
}

// Per-wave append: the lanes with `take` add their q to list at *len — one ballot and one
// atomicAdd by the leading lane per wave, the lanes scatter by their prefix popcount.  Every
// lane of the wave calls it (no early return before it for the lanes past a list's end).  A
// list's order therefore depends on which wave's atomicAdd lands first; no result does, since
// every output is indexed by q.  Nothing waits on another wave or block.
__device__ __forceinline__ void wave_append(bool take, uint64_t q, uint64_t* __restrict__ list,
                                            unsigned long long* len) {
  const uint64_t bal = __ballot(take);
  if (!bal) return;  // wave-uniform
  const uint32_t lane = threadIdx.x & 63, lead = (uint32_t)__ffsll((unsigned long long)bal) - 1u;
  unsigned long long base = 0;
  if (lane == lead) base = atomicAdd(len, (unsigned long long)__popcll(bal));
  base = __shfl(base, (int)lead);
  if (take) list[base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = q;
}

// Count within k <= K mismatches, per distance (cs_fm_count_mismatch_device): hist[q][d] = the
// summed exact counts of the strings at Hamming distance d from the pattern, d = 0..k, by
// mm_hist — at most K + 1 nested frames, all in registers.  K = 1 also
// serves k = 0, the exact count.  A lane whose tree is small idles until its wave's largest
// is done.
template <class E, int K>
__global__ __launch_bounds__(kBlk) void k_count_mm(DevIndex ix, const uint8_t* __restrict__ pats,
                                                   const uint64_t* __restrict__ offs, uint64_t npat,
                                                   uint32_t k, uint64_t* __restrict__ hist,
                                                   uint64_t fixed_m) {
  __shared__ NodeTable T;
  __shared__ SymList L;
  mm_stage<true>(T, L, ix);
  const uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (q >= npat) return;
  const MmPat p = mm_pattern(ix, pats, offs, fixed_m, q);
  uint64_t h[K + 1] = {};
  if (!p.search) h[0] = mm_unsearched(ix, p);
  else if (K == 1 && k == 0) h[0] = count_pattern<E>(ix, T, p.b, p.m);
  else mm_hist<E, K>(ix, T, L, p, h);
  uint64_t* const out = hist + q * (k + 1);
#pragma unroll
  for (int d = 0; d <= K; ++d)
    if ((uint32_t)d <= k) out[d] = h[d];
}

// Best stratum (cs_fm_best_mismatch_device): round K of launch_best_mm.  Round 0 is the exact
// count; a pattern of round K >= 1 has no hit at any distance below K, so the histogram's
// columns below K are zero and only hist[K] is taken.  A lane whose count is not zero writes
// (K, count); one without a hit appends its pattern to list_out (wave_append) or, in the last
// round, writes (CS_MM_NONE, 0).  So every pattern's outputs are written exactly once over the
// rounds.  list_out holds npat entries and receives at most *len_in <= npat.
template <class E, int K>
__global__ __launch_bounds__(kBlk) void k_best_mm(DevIndex ix, const uint8_t* __restrict__ pats,
                                                  const uint64_t* __restrict__ offs, uint64_t npat,
                                                  uint64_t fixed_m, bool last,
                                                  const uint64_t* __restrict__ list_in,
                                                  const unsigned long long* __restrict__ len_in,
                                                  uint64_t* __restrict__ list_out,
                                                  unsigned long long* len_out,
                                                  uint8_t* __restrict__ best_dist,
                                                  uint64_t* __restrict__ best_count) {
  uint64_t nlist;
  if (!mm_round_block<K>(npat, len_in, nlist)) return;
  __shared__ NodeTable T;
  __shared__ SymList L;
  mm_stage<(K > 0)>(T, L, ix);
  const uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  uint64_t q = 0;
  bool miss = false;
  if (e < nlist) {
    if constexpr (K > 0) q = list_in[e];
    else q = e;
    const MmPat p = mm_pattern(ix, pats, offs, fixed_m, q);
    uint64_t cnt = 0;
    if constexpr (K == 0) {
      cnt = p.search ? count_pattern<E>(ix, T, p.b, p.m) : mm_unsearched(ix, p);
    } else if (p.search) {
      uint64_t h[K + 1] = {};
      mm_hist<E, K>(ix, T, L, p, h);
      cnt = h[K];
    }
    miss = cnt == 0 && !last;
    if (!miss) {
      best_dist[q] = cnt ? (uint8_t)K : (uint8_t)CS_MM_NONE;
      best_count[q] = cnt;
    }
  }
  wave_append(miss, q, list_out, len_out);
}

// Locate within k <= K mismatches (cs_fm_locate_mismatch_device): the traversal of mm_leaves
// (fm_search.hpp; mm_hist's search with a leaf sink), run twice.  Sizing (kEmit = false): cnt_leaf[q] / cnt_occ[q] = the pattern's non-empty leaf
// ranges and the sum of their lengths (slot npat of both is zeroed for the scans' totals).
// Emitting (kEmit = true; cnt_leaf / cnt_occ now hold the exclusive scans, the second being the
// call's d_out_offs): leaf l, in traversal order from the pattern's first leaf, gets leaf_sp[l]
// (its first row: a plain locate record, bit 63 clear), leaf_off[l] (its offset in the output)
// and leaf_dist[l]; the thread after the last pattern writes the closing leaf_off[nleaf] =
// total.  The leaves are then the "patterns" of launch_locate_walk.  K = 1 also serves k = 0
// (mm_leaves' kmax).
template <class E, int K, bool kEmit>
__global__ __launch_bounds__(kBlk) void k_locate_mm(DevIndex ix, const uint8_t* __restrict__ pats,
                                                    const uint64_t* __restrict__ offs, uint64_t npat,
                                                    uint32_t k, uint64_t fixed_m, uint64_t* cnt_leaf,
                                                    uint64_t* cnt_occ, uint64_t* __restrict__ leaf_sp,
                                                    uint64_t* __restrict__ leaf_off,
                                                    uint8_t* __restrict__ leaf_dist, uint64_t nleaf,
                                                    uint64_t total) {
  __shared__ NodeTable T;
  __shared__ SymList L;
  mm_stage<true>(T, L, ix);
  const uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (q > npat) return;
  if (q == npat) {
    if (kEmit) leaf_off[nleaf] = total;
    else cnt_leaf[q] = cnt_occ[q] = 0;  // scan slots for the totals
    return;
  }
  const MmPat p = mm_pattern(ix, pats, offs, fixed_m, q);
  LeafSink sink = leaf_sink<kEmit>(q, cnt_leaf, cnt_occ, leaf_sp, leaf_off, leaf_dist);
  if (p.search) mm_leaves<E, 0, K>(ix, T, L, p.b, p.m, k, p.m, 0, ix.n, sink);
  if (!kEmit) {
    cnt_leaf[q] = sink.nleaf;
    cnt_occ[q] = sink.nocc;
  }
}

// Best-stratum locate (cs_fm_locate_best_mismatch_device): round K of
// launch_best_locate_mm_size / _emit; k_best_mm's rounds with k_locate_mm's two passes.  A
// pattern of round K has no hit below K, so its shallower subtrees die where they died before
// and every leaf the sink sees is a non-empty one at depth K: exactly stratum K, in the order
// k_locate_mm at the same bound visits those leaves.  The traversal is mm_leaves<E, 0, K> with
// kmax = K (K = 0: mm_rest, the exact search, and no symbol list is made).
// Sizing (kEmit = false): a lane with occurrences (in round 0 also an empty pattern over a
// non-empty text, with no leaf) writes best_dist[q] = K, cnt_leaf[q], cnt_occ[q] and appends q
// to the resolved list res at *res_len, a cursor shared by all rounds (the launch records it
// after each round, so round K's patterns are one slice of res).  A lane without a hit appends
// q to list_out or, in the last round, writes (CS_MM_NONE, 0, 0).  So every pattern's three
// values are written exactly once over the rounds.
// Emitting (kEmit = true): over round K's resolved slice list_in[0 .. nlist) (nlist from the
// host, the grid covers it; len_in and the append arguments are unused); leaf l of the pattern
// gets leaf_sp[l], leaf_off[l] and a distance byte nobody reads.  list_out and res hold npat
// entries each; a pattern enters at most one of them per round and res at most once.
template <class E, int K, bool kEmit>
__global__ __launch_bounds__(kBlk) void k_best_locate_mm(
    DevIndex ix, const uint8_t* __restrict__ pats, const uint64_t* __restrict__ offs, uint64_t npat,
    uint64_t fixed_m, bool last, const uint64_t* __restrict__ list_in,
    const unsigned long long* __restrict__ len_in, uint64_t nlist, uint64_t* __restrict__ list_out,
    unsigned long long* len_out, uint64_t* __restrict__ res, unsigned long long* res_len,
    uint8_t* __restrict__ best_dist, uint64_t* cnt_leaf, uint64_t* cnt_occ,
    uint64_t* __restrict__ leaf_sp, uint64_t* __restrict__ leaf_off, uint8_t* __restrict__ leaf_dist) {
  if constexpr (!kEmit)
    if (!mm_round_block<K>(npat, len_in, nlist)) return;
  __shared__ NodeTable T;
  __shared__ SymList L;
  mm_stage<(K > 0)>(T, L, ix);
  const uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  uint64_t q = 0;
  bool hit = false, miss = false;
  if (e < nlist) {
    if constexpr (K > 0 || kEmit) q = list_in[e];
    else q = e;
    const MmPat p = mm_pattern(ix, pats, offs, fixed_m, q);
    LeafSink sink = leaf_sink<kEmit>(q, cnt_leaf, cnt_occ, leaf_sp, leaf_off, leaf_dist);
    if (p.search) {
      if constexpr (K == 0) mm_rest<E>(ix, T, p.b, p.m, 0, p.m, 0, ix.n, sink);
      else mm_leaves<E, 0, K>(ix, T, L, p.b, p.m, (uint32_t)K, p.m, 0, ix.n, sink);
    }
    if constexpr (!kEmit) {
      hit = sink.nocc != 0 || (K == 0 && p.m == 0 && ix.n != 0);  // fm_index.cpp:80
      miss = !hit && !last;
      if (!miss) {
        best_dist[q] = hit ? (uint8_t)K : (uint8_t)CS_MM_NONE;
        cnt_leaf[q] = sink.nleaf;
        cnt_occ[q] = sink.nocc;
      }
    }
  }
  if constexpr (!kEmit) {
    wave_append(hit, q, res, res_len);
    wave_append(miss, q, list_out, len_out);
  }
}

// d_out_dist[leaf_off[l] .. leaf_off[l + 1]) = leaf_dist[l].  A lane fills a leaf of at most
// kLocSmall occurrences; the block's wider leaves (a 1-mer's holds n / 4 rows) are listed in
// LDS and filled by the whole block, one after the other.
__global__ __launch_bounds__(kBlk) void k_expand_dist(const uint64_t* __restrict__ leaf_off,
                                                      const uint8_t* __restrict__ leaf_dist,
                                                      uint64_t nleaf, uint8_t* __restrict__ out) {
  __shared__ uint32_t s_wide[kBlk];
  __shared__ uint32_t s_n;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const uint64_t l0 = blockIdx.x * (uint64_t)blockDim.x, l = l0 + threadIdx.x;
  if (l < nleaf) {
    const uint64_t a = leaf_off[l], b = leaf_off[l + 1];
    if (b - a <= kLocSmall) {
      const uint8_t d = leaf_dist[l];
      for (uint64_t i = a; i < b; ++i) out[i] = d;
    } else {
      s_wide[atomicAdd(&s_n, 1u)] = threadIdx.x;
    }
  }
  __syncthreads();
  const uint32_t nw = s_n;  // <= kBlk
  for (uint32_t e = 0; e < nw; ++e) {
    const uint64_t w = l0 + s_wide[e], a = leaf_off[w], b = leaf_off[w + 1];
    const uint8_t d = leaf_dist[w];
    for (uint64_t i = a + threadIdx.x; i < b; i += blockDim.x) out[i] = d;
  }
}

// ---- launch steps ----
// f(engine, K) for the handle's engine and the kernels of a bound k: K = k, and K = 1 for k = 0
template <class F>
void with_bound(const cs_fm_index* h, uint32_t k, F&& f) {
  with_engine(h->line_fmt, [&](auto engine) {
    with_int<2, 3, 1>((int)k, [&](auto K) { f(engine, K); });
  });
}

// The rounds of a best-stratum search: round(engine, K, r) for r = K = 0..k on the handle's
// engine, back to back; a round that returns an error ends them.
template <class F>
hipError_t with_rounds(const cs_fm_index* h, uint32_t k, F&& round) {
  hipError_t err = hipSuccess;
  with_engine(h->line_fmt, [&](auto engine) {
    for (uint32_t r = 0; r <= k && err == hipSuccess; ++r)
      with_int<0, 1, 2, 3>((int)r, [&](auto K) { err = round(engine, K, r); });
  });
  return err;
}

// The pending lists of those rounds: round r reads list r - 1 and appends to list r; the lists
// alternate between the two halves of `lists`, len[r] is list r's length (the owner's words,
// zeroed before round 0).  Round 0 reads no list and round k writes none.
struct PendingLists {
  StreamBuf lists;
  unsigned long long* len = nullptr;
  uint64_t npat = 0;
  uint32_t k = 0;
  hipError_t alloc(uint64_t npat_, uint32_t k_, hipStream_t st) {
    npat = npat_, k = k_;
    return k ? lists.alloc(2 * npat * 8, st) : hipSuccess;
  }
  const uint64_t* in(uint32_t r) const { return r ? lists.as<uint64_t>() + ((r - 1) & 1) * npat : nullptr; }
  const unsigned long long* len_in(uint32_t r) const { return r ? len + (r - 1) : nullptr; }
  uint64_t* out(uint32_t r) const { return r < k ? lists.as<uint64_t>() + (r & 1) * npat : nullptr; }
  unsigned long long* len_out(uint32_t r) const { return r < k ? len + r : nullptr; }
};

// A locate's sizing results per pattern, leaf[npat + 1] and occ[npat + 1] (slot npat zero),
// and their exclusive scans into plan.leaf_base and the call's d_out_offs, whose slot npat
// then holds the totals: copied to *nleaf_to and *total_to (host or device words, `kind`).
struct LeafCounts {
  StreamBuf leaf, occ, tmp;
  cs_status alloc(uint64_t npat, MmLeafPlan& plan, hipStream_t st) {
    FMX_HIP(leaf.alloc((npat + 1) * 8, st));
    FMX_HIP(occ.alloc((npat + 1) * 8, st));
    FMX_HIP(plan.leaf_base.alloc((npat + 1) * 8, st));
    return CS_OK;
  }
  cs_status scan(uint64_t npat, uint64_t* d_out_offs, MmLeafPlan& plan, void* total_to, void* nleaf_to,
                 hipMemcpyKind kind, hipStream_t st) {
    // one temporary serves both scans: same type, same length
    size_t tb = 0;
    FMX_HIP(rocprim::exclusive_scan(nullptr, tb, occ.as<uint64_t>(), d_out_offs, (uint64_t)0, npat + 1,
                                    rocprim::plus<uint64_t>(), st));
    FMX_HIP(tmp.alloc(tb, st));
    FMX_HIP(rocprim::exclusive_scan(tmp.p, tb, occ.as<uint64_t>(), d_out_offs, (uint64_t)0, npat + 1,
                                    rocprim::plus<uint64_t>(), st));
    FMX_HIP(rocprim::exclusive_scan(tmp.p, tb, leaf.as<uint64_t>(), plan.leaf_base.as<uint64_t>(),
                                    (uint64_t)0, npat + 1, rocprim::plus<uint64_t>(), st));
    FMX_HIP(hipMemcpyAsync(total_to, d_out_offs + npat, 8, kind, st));
    FMX_HIP(hipMemcpyAsync(nleaf_to, plan.leaf_base.as<uint64_t>() + npat, 8, kind, st));
    return CS_OK;
  }
};

// Positions from a leaf list: leaf l has its first row sp[l], its place in the output
// off[l] (off[nleaf] = total) and its distance dist[l]; the overrun word starts as "none".
struct LeafList {
  StreamBuf sp, off, dist, err;
  cs_status alloc(uint64_t nleaf, hipStream_t st) {
    FMX_HIP(sp.alloc(nleaf * 8, st));
    FMX_HIP(off.alloc((nleaf + 1) * 8, st));
    FMX_HIP(dist.alloc(nleaf, st));
    FMX_HIP(err.alloc(8, st));
    FMX_HIP(hipMemsetAsync(err.p, 0xFF, 8, st));
    return CS_OK;
  }
  // The exact locate's phase 2 with the leaves as its patterns into d_out_pos[total] (the
  // leaves are in pattern order, so the output is in batch order), the leaves' distances into
  // d_out_dist[total] when the call has such an output, then the overrun word is read
  // (synchronises st).  ev: null, or the phase events 4 and 5 of launch_locate_mm_emit.
  cs_status positions(const cs_fm_index* h, uint64_t nleaf, uint64_t total, uint64_t* d_out_pos,
                      uint8_t* d_out_dist, uint32_t flags, hipStream_t st, hipEvent_t* ev) {
    unsigned long long* e = err.as<unsigned long long>();
    cs_status s = launch_locate_walk(h, sp.as<uint64_t>(), off.as<uint64_t>(), nleaf, total, d_out_pos, st,
                                     e, flags);
    if (s != CS_OK) return s;
    if (ev) FMX_HIP(hipEventRecord(ev[4], st));
    if (d_out_dist && nleaf) {
      k_expand_dist<<<grid_for(nleaf, kBlk, 0xFFFFFFFFu), kBlk, 0, st>>>(
          off.as<uint64_t>(), dist.as<uint8_t>(), nleaf, d_out_dist);
      FMX_HIP(hipGetLastError());
    }
    if (ev) FMX_HIP(hipEventRecord(ev[5], st));
    return check_locate_error(h, e, st);
  }
};

}  // namespace

cs_status launch_count_mm(const cs_fm_index* h, const uint8_t* d_pats, const uint64_t* d_offs,
                          uint64_t npat, uint32_t k, uint64_t* d_hist, uint32_t flags, hipStream_t st,
                          uint64_t fixed_m) {
  if (!npat) return CS_OK;
  const DevIndex ix = query_dev(h, call_flags(h, flags));
  const unsigned g = grid_for(npat, kBlk, 0xFFFFFFFFu);
  with_bound(h, k, [&](auto engine, auto K) {
    using E = typename decltype(engine)::type;
    k_count_mm<E, K><<<g, kBlk, 0, st>>>(ix, d_pats, d_offs, npat, k, d_hist, fixed_m);
  });
  FMX_HIP(hipGetLastError());
  return CS_OK;
}

cs_status launch_best_mm(const cs_fm_index* h, const uint8_t* d_pats, const uint64_t* d_offs,
                         uint64_t npat, uint32_t k, uint8_t* d_best_dist, uint64_t* d_best_count,
                         uint32_t flags, hipStream_t st, uint64_t fixed_m) {
  if (!npat) return CS_OK;
  PendingLists pend;
  StreamBuf len;
  FMX_HIP(pend.alloc(npat, k, st));
  if (k) {
    FMX_HIP(len.alloc(CS_MM_MAX * 8, st));
    FMX_HIP(hipMemsetAsync(len.p, 0, CS_MM_MAX * 8, st));
  }
  pend.len = len.as<unsigned long long>();
  const DevIndex ix = query_dev(h, call_flags(h, flags));
  // a round's list length is known on the device only: every round's grid covers npat
  const unsigned g = grid_for(npat, kBlk, 0xFFFFFFFFu);
  (void)with_rounds(h, k, [&](auto engine, auto K, uint32_t r) {
    using E = typename decltype(engine)::type;
    k_best_mm<E, K><<<g, kBlk, 0, st>>>(ix, d_pats, d_offs, npat, fixed_m, /*last*/ r == k, pend.in(r),
                                        pend.len_in(r), pend.out(r), pend.len_out(r), d_best_dist,
                                        d_best_count);
    return hipSuccess;
  });
  FMX_HIP(hipGetLastError());
  return CS_OK;
}

cs_status launch_locate_mm_size(const cs_fm_index* h, const uint8_t* d_pats, const uint64_t* d_offs,
                                uint64_t npat, uint32_t k, uint64_t fixed_m, uint64_t* d_out_offs,
                                uint32_t flags, hipStream_t st, MmLeafPlan& plan, hipEvent_t* ev) {
  LeafCounts cnt;
  cs_status s = cnt.alloc(npat, plan, st);
  if (s != CS_OK) return s;
  const DevIndex ix = query_dev(h, call_flags(h, flags));
  const unsigned g = grid_for(npat + 1, kBlk, 0xFFFFFFFFu);
  if (ev) FMX_HIP(hipEventRecord(ev[0], st));
  with_bound(h, k, [&](auto engine, auto K) {
    using E = typename decltype(engine)::type;
    k_locate_mm<E, K, false><<<g, kBlk, 0, st>>>(ix, d_pats, d_offs, npat, k, fixed_m,
                                                 cnt.leaf.as<uint64_t>(), cnt.occ.as<uint64_t>(), nullptr,
                                                 nullptr, nullptr, 0, 0);
  });
  FMX_HIP(hipGetLastError());
  if (ev) FMX_HIP(hipEventRecord(ev[1], st));
  if ((s = cnt.scan(npat, d_out_offs, plan, &plan.total, &plan.nleaf, hipMemcpyDeviceToHost, st)) != CS_OK)
    return s;
  if (ev) FMX_HIP(hipEventRecord(ev[2], st));
  FMX_HIP(hipStreamSynchronize(st));
  return CS_OK;
}

cs_status launch_locate_mm_emit(const cs_fm_index* h, const uint8_t* d_pats, const uint64_t* d_offs,
                                uint64_t npat, uint32_t k, uint64_t fixed_m,
                                const uint64_t* d_out_offs, const MmLeafPlan& plan,
                                uint64_t* d_out_pos, uint8_t* d_out_dist, uint32_t flags,
                                hipStream_t st, hipEvent_t* ev) {
  LeafList leaves;
  cs_status s = leaves.alloc(plan.nleaf, st);
  if (s != CS_OK) return s;
  const DevIndex ix = query_dev(h, call_flags(h, flags));
  const unsigned g = grid_for(npat + 1, kBlk, 0xFFFFFFFFu);
  with_bound(h, k, [&](auto engine, auto K) {
    using E = typename decltype(engine)::type;
    k_locate_mm<E, K, true><<<g, kBlk, 0, st>>>(
        ix, d_pats, d_offs, npat, k, fixed_m, plan.leaf_base.as<uint64_t>(),
        const_cast<uint64_t*>(d_out_offs), leaves.sp.as<uint64_t>(), leaves.off.as<uint64_t>(),
        leaves.dist.as<uint8_t>(), plan.nleaf, plan.total);
  });
  FMX_HIP(hipGetLastError());
  if (ev) FMX_HIP(hipEventRecord(ev[3], st));
  return leaves.positions(h, plan.nleaf, plan.total, d_out_pos, d_out_dist, flags, st, ev);
}

cs_status launch_best_locate_mm_size(const cs_fm_index* h, const uint8_t* d_pats,
                                     const uint64_t* d_offs, uint64_t npat, uint32_t k,
                                     uint64_t fixed_m, uint8_t* d_best_dist, uint64_t* d_out_offs,
                                     uint32_t flags, hipStream_t st, BestLeafPlan& plan) {
  // control words: [0, CS_MM_MAX) the pending lists' lengths, then the resolved list's cursor,
  // and what the host reads back in one copy: bound[0 .. CS_MM_MAX + 2) (those past k + 1 stay
  // 0 and are not used), total, nleaf
  constexpr uint32_t kCur = CS_MM_MAX, kBound = kCur + 1, kTotal = kBound + CS_MM_MAX + 2,
                     kWords = kTotal + 2;
  LeafCounts cnt;
  PendingLists pend;
  StreamBuf ctl;
  cs_status s = cnt.alloc(npat, plan, st);
  if (s != CS_OK) return s;
  FMX_HIP(plan.res.alloc(npat * 8, st));
  FMX_HIP(pend.alloc(npat, k, st));
  FMX_HIP(ctl.alloc(kWords * 8, st));
  FMX_HIP(hipMemsetAsync(ctl.p, 0, kWords * 8, st));
  // scan slots for the totals
  FMX_HIP(hipMemsetAsync(cnt.leaf.as<uint64_t>() + npat, 0, 8, st));
  FMX_HIP(hipMemsetAsync(cnt.occ.as<uint64_t>() + npat, 0, 8, st));
  const DevIndex ix = query_dev(h, call_flags(h, flags));
  unsigned long long* const w = ctl.as<unsigned long long>();
  pend.len = w;
  // a round's list length is known on the device only: every round's grid covers npat
  const unsigned g = grid_for(npat, kBlk, 0xFFFFFFFFu);
  const hipError_t rounds = with_rounds(h, k, [&](auto engine, auto K, uint32_t r) {
    using E = typename decltype(engine)::type;
    k_best_locate_mm<E, K, false><<<g, kBlk, 0, st>>>(
        ix, d_pats, d_offs, npat, fixed_m, /*last*/ r == k, pend.in(r), pend.len_in(r), 0, pend.out(r),
        pend.len_out(r), plan.res.as<uint64_t>(), w + kCur, d_best_dist, cnt.leaf.as<uint64_t>(),
        cnt.occ.as<uint64_t>(), nullptr, nullptr, nullptr);
    // round r's patterns are res[bound[r] .. bound[r + 1])
    return hipMemcpyAsync(w + kBound + r + 1, w + kCur, 8, hipMemcpyDeviceToDevice, st);
  });
  FMX_HIP(rounds);
  FMX_HIP(hipGetLastError());
  // one read-back: the bounds and the two totals
  if ((s = cnt.scan(npat, d_out_offs, plan, w + kTotal, w + kTotal + 1, hipMemcpyDeviceToDevice, st)) != CS_OK)
    return s;
  uint64_t back[CS_MM_MAX + 4];
  FMX_HIP(hipMemcpyAsync(back, w + kBound, sizeof back, hipMemcpyDeviceToHost, st));
  FMX_HIP(hipStreamSynchronize(st));
  for (uint32_t r = 0; r < CS_MM_MAX + 2; ++r) plan.bound[r] = back[r];
  plan.total = back[CS_MM_MAX + 2];
  plan.nleaf = back[CS_MM_MAX + 3];
  return CS_OK;
}

cs_status launch_best_locate_mm_emit(const cs_fm_index* h, const uint8_t* d_pats,
                                     const uint64_t* d_offs, uint64_t npat, uint32_t k,
                                     uint64_t fixed_m, const uint64_t* d_out_offs,
                                     const BestLeafPlan& plan, uint64_t* d_out_pos, uint32_t flags,
                                     hipStream_t st) {
  LeafList leaves;  // (its distance bytes: all K in round K, unread)
  cs_status s = leaves.alloc(plan.nleaf, st);
  if (s != CS_OK) return s;
  const DevIndex ix = query_dev(h, call_flags(h, flags));
  (void)with_rounds(h, k, [&](auto engine, auto K, uint32_t r) {
    using E = typename decltype(engine)::type;
    const uint64_t nres = plan.bound[r + 1] - plan.bound[r];
    if (nres)
      k_best_locate_mm<E, K, true><<<grid_for(nres, kBlk, 0xFFFFFFFFu), kBlk, 0, st>>>(
          ix, d_pats, d_offs, npat, fixed_m, false, plan.res.as<uint64_t>() + plan.bound[r], nullptr, nres,
          nullptr, nullptr, nullptr, nullptr, nullptr, plan.leaf_base.as<uint64_t>(),
          const_cast<uint64_t*>(d_out_offs), leaves.sp.as<uint64_t>(), leaves.off.as<uint64_t>(),
          leaves.dist.as<uint8_t>());
    return hipSuccess;
  });
  FMX_HIP(hipGetLastError());
  // the closing leaf_off[nleaf] = total
  FMX_HIP(hipMemcpyAsync(leaves.off.as<uint64_t>() + plan.nleaf, d_out_offs + npat, 8,
                         hipMemcpyDeviceToDevice, st));
  return leaves.positions(h, plan.nleaf, plan.total, d_out_pos, nullptr, flags, st, nullptr);
}

}  // namespace fmx

// fm_locate.hip — the finish of the one-call locate (fm_locate.hpp): after the search kernels
// (fm_query.hip) have written a count and a record per pattern and a total per tile, the
// tile scan (2), the emit (3), the listed walks (3') and the wide ranges; the call's buffer
// layout and the launches.
#include "fm_locate.hpp"

namespace fmx {
namespace {

// (2) past kScanMaxBlocks kScanBlock = 2^20 tiles (more than 536,870,912 patterns; below,
// k_scan_chained): exclusive scan of the tile totals in place, one block; total ->
// *total_out.  No test reaches that size, so the body is as it was measured in round 5.  The
// tiles pass through LDS 16 k at a time (128 KB + padding: a workgroup may hold 160 KB), so
// the global loads and stores are coalesced — the round-3 form gave each thread 32
// consecutive tiles straight from memory (strided loads and stores: 28 us for C4's 24 k
// tiles) — then each thread scans a contiguous run of 16 in registers and the block scans
// the run totals.
__device__ __forceinline__ uint32_t scan_pad(uint32_t i) { return i + (i >> 4); }  // LDS bank spread
__global__ __launch_bounds__(1024) void k_scan_tiles(uint64_t* __restrict__ tiles, uint64_t ntiles,
                                                     uint64_t* __restrict__ total_out) {
  constexpr int kRun = 16;                     // tiles per thread per round
  constexpr uint32_t kChunk = 1024u * kRun;    // tiles per round
  __shared__ uint64_t s_v[kChunk + kChunk / kRun];
  __shared__ uint64_t s_w[16];
  __shared__ uint64_t s_carry;
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (t == 0) s_carry = 0;
  for (uint64_t b = 0; b < ntiles; b += kChunk) {
#pragma unroll
    for (int r = 0; r < kRun; ++r) {  // coalesced: tile b + r 1024 + t
      const uint64_t i = b + (uint64_t)r * 1024 + t;
      s_v[scan_pad(r * 1024u + t)] = i < ntiles ? tiles[i] : 0ull;
    }
    __syncthreads();
    uint64_t v[kRun], run = 0;
#pragma unroll
    for (int r = 0; r < kRun; ++r) {  // the thread's run: tiles b + t kRun + r
      v[r] = s_v[scan_pad(t * kRun + r)];
      run += v[r];
    }
    uint64_t x = run;  // inclusive scan of the run totals over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t y = __shfl_up(x, d, 64);
      if (lane >= (uint32_t)d) x += y;
    }
    if (lane == 63) s_w[wv] = x;
    __syncthreads();
    uint64_t pre = 0, tot = 0;
#pragma unroll
    for (int w2 = 0; w2 < 16; ++w2) {
      if (w2 < (int)wv) pre += s_w[w2];
      tot += s_w[w2];
    }
    uint64_t acc = s_carry + pre + x - run;
#pragma unroll
    for (int r = 0; r < kRun; ++r) {
      s_v[scan_pad(t * kRun + r)] = acc;
      acc += v[r];
    }
    __syncthreads();  // (every thread has read s_carry and s_w of this round)
    if (t == 0) s_carry += tot;
#pragma unroll
    for (int r = 0; r < kRun; ++r) {
      const uint64_t i = b + (uint64_t)r * 1024 + t;
      if (i < ntiles) tiles[i] = s_v[scan_pad(r * 1024u + t)];
    }
    __syncthreads();  // before the next round's loads overwrite s_v and its scan reads s_carry
  }
  if (t == 0) *total_out = s_carry;
}

// (2): the exclusive scan of the tile totals in place over ceil(ntiles / 1024) blocks of 1024
// tiles (one per thread): each block publishes its total (one flag word), sums its
// predecessors' — every thread polls one of them — and writes its tiles' exclusive prefixes;
// the last block writes the total.  The
// blocks wait only on lower ones.  (Round 5: the one-block scan took 18 us of C4's 0.53-ms
// one-call locate, its 24 k tiles passing through one CU.)  A block's place in the chain is
// the order in which it STARTS (an atomic ticket, sflags[kScanMaxBlocks], zeroed by the
// search kernel with the flags), not its blockIdx: a block only ever waits on blocks that
// are already running, whatever order the dispatcher picks (with other streams'
// kernels sharing the CUs, blockIdx order is not guaranteed).
__global__ __launch_bounds__(kScanBlock) void k_scan_chained(uint64_t* __restrict__ tiles, uint64_t ntiles,
                                                             uint64_t* __restrict__ total_out,
                                                             unsigned long long* __restrict__ sflags) {
  __shared__ uint64_t s_w[kScanBlock / 64];
  __shared__ uint64_t s_p[kScanBlock / 64];
  __shared__ uint32_t s_id;
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (t == 0) s_id = (uint32_t)atomicAdd(sflags + kScanMaxBlocks, 1ull);
  __syncthreads();
  const uint32_t bid = s_id;
  const uint64_t i = (uint64_t)bid * kScanBlock + t;
  const uint64_t v = i < ntiles ? tiles[i] : 0ull;
  uint64_t agg;
  const uint64_t pre = block_scan_excl<uint64_t, kScanBlock / 64>(v, s_w, agg);
  if (t == 0)
    __hip_atomic_store(sflags + bid, (1ull << 63) | agg, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  uint64_t p = 0;  // predecessor t's total
  if (t < bid) {
    unsigned long long f;
    do {
      f = __hip_atomic_load(sflags + t, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
    } while (!(f >> 63));
    p = f & ~(1ull << 63);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) p += __shfl_xor(p, d, 64);
  if (lane == 0) s_p[wv] = p;
  __syncthreads();
  uint64_t base = 0;
#pragma unroll
  for (int w2 = 0; w2 < (int)(kScanBlock / 64); ++w2) base += s_p[w2];
  if (i < ntiles) tiles[i] = base + pre;
  if (bid == gridDim.x - 1 && t == 0) *total_out = base + agg;
}

// (3)'s decision for pattern q, reporting c = min(count, limit) positions from output index
// a, record s: stores its offset; a stashed position is stored; a window or a range of at most
// kLocSmall rows returns c, the rows the caller produces; a wider range is appended to the
// wide list (k_locate_emit_wide).  0: nothing more to do for the pattern.
__device__ __forceinline__ uint64_t emit_pattern(const OnePass& op, uint64_t q, uint64_t a, uint64_t c,
                                                 uint64_t s) {
  st_out(op.out_offs + q, a);
  if (!c || a + c > op.cap) return 0;  // capacity short: the caller sees the total
  if (loc_stashed(s)) {  // kLocStash: the one position, read by the search kernel
    st_out(op.out_pos + a, s & (kLocStash - 1));
    return 0;
  }
  if ((s & kLocCtx) || c <= kLocSmall) return c;  // (a window k characters before the end: k_locate_sa)
  const unsigned long long e = atomicAdd(op.nwide, 1ull);
  if (e < op.wide_cap) {
    op.wide[2 * e] = q;
    op.wide[2 * e + 1] = s;
  }
  return 0;
}

// the positions of a record's first c <= kLocSmall reported rows, minus the window's adj
// (mod n), to out: SA reads kEmitRows at a time, in flight together
// (the walk-line forms list their rows instead: emit_walk_lines)
constexpr int kEmitRows = 4;
template <int kPos>
__device__ __forceinline__ void emit_rows(const DevIndex& ix, const NodeTable& T, const OnePass& op,
                                          uint64_t* __restrict__ out, uint64_t c, LocRows rows) {
  const uint64_t n = ix.n, adj = rows.adj;
  for (uint64_t i = 0; i < c; i += kEmitRows) {
    uint64_t row[kEmitRows];
    bool act[kEmitRows];
#pragma unroll
    for (int u = 0; u < kEmitRows; ++u) {
      act[u] = i + u < c;
      row[u] = act[u] ? rows.next() : 0;
    }
    static_assert(kPos == 0, "walk-line indexes list their rows (emit_walk_lines)");
#pragma unroll
    for (int u = 0; u < kEmitRows; ++u)
      if (act[u]) row[u] = load_sa(op.sa, row[u]);
#pragma unroll
    for (int u = 0; u < kEmitRows; ++u)
      if (act[u]) st_out(out + i + u, pos_back(row[u], adj, n));
  }
}

// (3) on walk-line indexes: offsets, the stashed positions, and the rows of every pattern
// with 2..kLocSmall positions listed for k_locate_walks in the tile's slots (a block scan
// places them: no atomic) instead of walked here — a lane walking its pattern's positions
// one after another kept its wave, and the emit, waiting (C5: the emit 360 us per 12.5 M
// 20-mers; 617 with four walks of a lane in lockstep; 1,156 with one global list counter,
// 98 k same-address atomics, profiles/r05/r05x, r05y).  A pattern past the tile's kLocTile
// slots is walked here (its slots below the limit marked void).
template <int U, int kPos>
__device__ __forceinline__ void emit_walk_lines(const DevIndex& ix, NodeTable& T, uint64_t npat, uint64_t tile,
                                                uint64_t q0, const uint64_t* kc, const uint64_t* kr,
                                                const uint64_t* mine, uint64_t base, const OnePass& op) {
  const uint64_t n = ix.n;
  uint64_t nl[U], tot = 0;
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const uint64_t q = q0 + (uint64_t)j * kBlk;
    nl[j] = q < npat ? emit_pattern(op, q, base + mine[j], kc[j], kr[j]) : 0;
    tot += nl[j];
  }
  // the lane's place among the tile's listed rows
  uint64_t at, all;
  block_scan<1>(&tot, &at, all);
  if (threadIdx.x == 0) op.wcnt[tile] = (uint32_t)(all < kLocTile ? all : kLocTile);
  uint64_t* const slots = op.walks + 2 * tile * kLocTile;
  uint32_t fb = 0;  // patterns walked here (past the tile's slots)
#pragma unroll
  for (int j = 0; j < U; ++j) {
    if (!nl[j]) continue;
    const uint64_t a = base + mine[j], s = kr[j], c = nl[j];
    const bool fits = at + c <= kLocTile;
    fb |= (uint32_t)!fits << j;
    LocRows rows = LocRows::of(s);
    for (uint64_t i = 0; i < c; ++i, ++at) {
      const uint64_t row = rows.next();
      if (at >= kLocTile) continue;
      slots[2 * at] = fits ? a + i : ~0ull;  // (a void slot: k_locate_walks skips it)
      slots[2 * at + 1] = row | (rows.adj << kWalkAdjShift);
    }
  }
  if (__syncthreads_or(fb != 0)) {
    load_table(T, ix.table);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < U; ++j) {
      if (!((fb >> j) & 1u)) continue;
      const uint64_t a = base + mine[j];
      LocRows rows = LocRows::of(kr[j]);
      const uint64_t adj = rows.adj;
      for (uint64_t i = 0; i < nl[j]; ++i)
        st_out(op.out_pos + a + i, pos_back(walk_position<WalkLineOf<kPos>>(ix, T, rows.next()), adj, n));
    }
  }
}

// (3') the listed walks (emit_walk_lines): block b takes tiles b, b + grid, ... (one per
// thread: the grid is at least tiles / kBlk), their slots flattened, two per lane in lockstep
template <int kPos>
__global__ __launch_bounds__(kBlk) void k_locate_walks(DevIndex ix, OnePass op, uint64_t ntiles) {
  __shared__ NodeTable T;
  __shared__ uint32_t s_off[kBlk + 1];
  __shared__ uint32_t s_w[kBlk / 64];
  const uint64_t mt = blockIdx.x + (uint64_t)threadIdx.x * gridDim.x;
  const uint32_t tot = slot_offsets(mt < ntiles ? op.wcnt[mt] : 0u, s_off, s_w);
  if (tot == 0) return;  // uniform: nothing listed in the block's tiles
  load_table(T, ix.table);
  __syncthreads();
  const uint64_t n = ix.n;
  slot_entries<2>(s_off, tot, [&](const uint32_t* owner, const uint32_t* place, const bool* live) {
    uint64_t row[2], adj[2], idx[2];
    bool act[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint64_t* sl = op.walks + 2 * ((blockIdx.x + (uint64_t)owner[h] * gridDim.x) * kLocTile + place[h]);
      idx[h] = live[h] ? sl[0] : ~0ull;
      const uint64_t v = live[h] ? sl[1] : 0;
      act[h] = idx[h] != ~0ull;
      row[h] = v & kWalkRowMask;
      adj[h] = v >> kWalkAdjShift;
    }
    bool w[2] = {act[0], act[1]};
    walk_positions<WalkLineOf<kPos>, 2>(ix, T, row, w);
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (act[h]) st_out(op.out_pos + idx[h], pos_back(row[h], adj[h], n));
  });
}

// (3): offsets and positions of tile blockIdx.x (round 5: a pattern whose record is a stashed
// position has no count stored: 8 B read per pattern instead of 12.  Tried in round 5 to drop
// the scan kernel: a decoupled look-back over the tiles — its frontier moves 64 tiles per L2
// round trip, 0.63 against 0.53 ms per C4 call — 1024 blocks taking a share of the tiles each
// with a running base — 4 waves per SIMD and a serial tile loop, the emit 125 against 67 us
// — share totals added by the search kernel's waves — same-address atomics of
// neighbouring blocks, the search 426 -> 615 us — and two tiles per block, 4 patterns per
// lane with both tiles' records in flight before one scan: 0.520 -> 0.536 ms per call,
// profiles/r05/r05aj.)
template <int U, int kPos = 0>
__global__ __launch_bounds__(kBlk) void k_locate_emit(DevIndex ix, uint64_t npat, OnePass op) {
  __shared__ NodeTable T;  // kPos: the walks' C[] and codes (a pattern past walk_cap)
  const uint64_t tile = blockIdx.x;
  const uint64_t q0 = tile * (uint64_t)(kBlk * U) + threadIdx.x;
  uint64_t kc[U], kr[U], mine[U], agg;
  const uint64_t base = op.tiles[tile];  // (issued with the records: its latency overlaps theirs)
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const uint64_t q = q0 + (uint64_t)j * kBlk;
    // (read once: non-temporal loads, 0.560 -> 0.554 ms per call over three A/B rounds,
    // profiles/r04/ab_lib_r04af.jsonl); the count only where the record is no stash
    kr[j] = q < npat ? __builtin_nontemporal_load(op.rec + q) : 0;
    kc[j] = q >= npat ? 0 : loc_stashed(kr[j]) ? 1
          : (op.cnt64 ? __builtin_nontemporal_load(op.cnt64 + q) : __builtin_nontemporal_load(op.cnt + q));
  }
  block_scan<U>(kc, mine, agg);
  if constexpr (kPos != 0) {
    emit_walk_lines<U, kPos>(ix, T, npat, tile, q0, kc, kr, mine, base, op);
  } else {
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const uint64_t q = q0 + (uint64_t)j * kBlk;
      if (q >= npat) continue;
      const uint64_t a = base + mine[j];
      const uint64_t c = emit_pattern(op, q, a, kc[j], kr[j]), s = kr[j];
      if (!c) continue;
      if (s & kLocCtx) emit_rows<kPos>(ix, T, op, op.out_pos + a, c, LocRows::of(s));
      else emit_rows<kPos>(ix, T, op, op.out_pos + a, c, LocRows(s));
    }
  }
}

// the ranges over kLocSmall rows: a block per range
template <int kPos = 0>
__global__ __launch_bounds__(kBlk) void k_locate_emit_wide(DevIndex ix, OnePass op, const uint64_t* __restrict__ offs,
                                                           uint64_t* __restrict__ out) {
  __shared__ NodeTable T;
  const uint64_t nw = *op.nwide < op.wide_cap ? *op.nwide : op.wide_cap;
  if (blockIdx.x >= nw) return;  // uniform over the block
  if constexpr (kPos != 0) {
    load_table(T, ix.table);
    __syncthreads();
  }
  for (uint64_t e = blockIdx.x; e < nw; e += gridDim.x) {
    const uint64_t q = op.wide[2 * e], s = op.wide[2 * e + 1], a = offs[q], c = offs[q + 1] - a;
    for (uint64_t j = threadIdx.x; j < c; j += blockDim.x) st_out(out + a + j, onepass_pos<kPos>(ix, T, op, s + j));
  }
}

// Where each part of the call's buffers sits (byte offsets from their start, after the
// lists) and the total: the one description the workspace sizes and locate_buffers' pointers
// share.
struct LocateLayout {
  uint64_t ntiles;  // tiles of kLocTile patterns
  uint64_t rec, tiles, nwide, wide, counts, wcnt, walks, sflags, bytes;
  LocateLayout(const cs_fm_index* h, uint64_t npat, uint64_t wide_cap) {
    ntiles = (npat + kLocTile - 1) / kLocTile;
    const uint64_t cb = h->wide ? 8 : 4;  // count bytes (a wide index's counts pass 2^32)
    const bool walk = !h->d_sa;           // a walk-line index: the walk list
    rec = 0;                                              // a record per pattern, 8 B
    tiles = rec + npat * 8;                               // a total per tile, 8 B
    nwide = tiles + ntiles * 8;                           // the wide ranges' counter, 8 B
    wide = nwide + 8;                                     // wide_cap wide ranges, 16 B each
    counts = wide + wide_cap * 16;                        // a count per pattern, cb bytes
    wcnt = counts + ((npat * cb + 7) & ~7ull);            // the tiles' walk counts, u32
    walks = wcnt + (walk ? (ntiles * 4 + 7) & ~7ull : 0);  // kLocTile 16-B walk slots per tile
    sflags = walks + (walk ? ntiles * kLocTile * 16 : 0);  // the chained scan's flags and ticket
    bytes = sflags + (kScanMaxBlocks + 1) * 8;
  }
};

}  // namespace

uint64_t locate_workspace_bytes(const cs_fm_index* h, uint64_t npat) {
  return count_workspace_bytes(h, npat) + LocateLayout(h, npat, npat).bytes;
}

cs_status locate_buffers(const cs_fm_index* h, uint64_t npat, uint64_t wide_cap, uint64_t ws_lists,
                         uint64_t lists, const Work& work, hipStream_t st, LocateBufs& b) {
  const LocateLayout L(h, npat, wide_cap);
  b.in_ws = work.p && work.bytes >= ws_lists + L.bytes;
  uint64_t lo_at;
  if (b.in_ws) {
    b.base = static_cast<uint8_t*>(work.p);
    lo_at = ws_lists;
  } else {
    FMX_HIP(b.own.alloc(lists + L.bytes, st));
    b.base = b.own.as<uint8_t>();
    lo_at = lists;
  }
  OnePass& op = b.op;
  uint8_t* const lp = b.base + lo_at;
  op.rec = reinterpret_cast<uint64_t*>(lp + L.rec);
  op.tiles = reinterpret_cast<uint64_t*>(lp + L.tiles);
  op.nwide = reinterpret_cast<unsigned long long*>(lp + L.nwide);
  op.wide = reinterpret_cast<uint64_t*>(lp + L.wide);
  if (h->wide) op.cnt64 = reinterpret_cast<uint64_t*>(lp + L.counts);
  else op.cnt = reinterpret_cast<uint32_t*>(lp + L.counts);
  // (walk-line indexes, kPos 1 / 2: launch_locate_onepass takes an index without the full
  // suffix array only by its walk lines, so !d_sa is kpos != 0 — and LocateLayout's `walk`)
  if (!h->d_sa) {
    op.wcnt = reinterpret_cast<uint32_t*>(lp + L.wcnt);
    op.walks = reinterpret_cast<uint64_t*>(lp + L.walks);
  }
  op.sflags = reinterpret_cast<unsigned long long*>(lp + L.sflags);
  op.sa = static_cast<const uint32_t*>(h->d_sa);
  op.wide_cap = wide_cap;
  return CS_OK;
}

cs_status launch_locate_finish(const DevIndex& ix, uint64_t npat, uint64_t tiles, int kpos,
                               const OnePass& op, uint64_t* total, hipStream_t st) {
  constexpr int U = kLocTile / kBlk;  // (the emit's tiles are the search kernels')
  // (k_locate_walks: 4 blocks per CU, and one tile per thread)
  const unsigned walk_grid = (unsigned)std::max<uint64_t>(list_blocks_per_device(), (tiles + kBlk - 1) / kBlk);
  // the chained scan (a block per 1024 tiles) while its look-back fits a block, else one block
  const uint64_t sblocks = (tiles + kScanBlock - 1) / kScanBlock;
  if (sblocks <= kScanMaxBlocks)
    k_scan_chained<<<(unsigned)sblocks, kScanBlock, 0, st>>>(op.tiles, tiles, op.out_offs + npat, op.sflags);
  else
    k_scan_tiles<<<1, 1024, 0, st>>>(op.tiles, tiles, op.out_offs + npat);
  FMX_HIP(hipGetLastError());
  // kPos: positions from the full SA (0), or by the walk over narrow (1) / wide (2) walk lines
  with_int<0, 1, 2>(kpos, [&](auto kPos) {
    k_locate_emit<U, kPos><<<(unsigned)tiles, kBlk, 0, st>>>(ix, npat, op);
    if constexpr (kPos != 0) k_locate_walks<kPos><<<walk_grid, kBlk, 0, st>>>(ix, op, tiles);
    k_locate_emit_wide<kPos><<<1024, kBlk, 0, st>>>(ix, op, op.out_offs, op.out_pos);
  });
  FMX_HIP(hipGetLastError());
  FMX_HIP(hipMemcpyAsync(total, op.out_offs + npat, 8, hipMemcpyDeviceToHost, st));
  FMX_HIP(hipStreamSynchronize(st));
  return CS_OK;
}

}  // namespace fmx

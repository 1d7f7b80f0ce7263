// fm_locate.hpp — the one-call locate (cs_fm_locate_device's single launch sequence): the
// contract between its searches (fm_query.hip) and its finish (fm_locate.hip).
//
// Batch locate in one call over an index that keeps the full suffix array: the search, the
// finish's three launches and one host synchronisation —
//   (1) the search (fm_query.hip): k_count_ctx with kOne, the staged search — or
//       k_count_qctx with kOne, k_locate_one_gen, k_locate_long, k_locate_list — writes per
//       pattern its record and, unless the record is the pattern's only position (kLocStash
//       below: count 1, 99.6 % of C4 Q_text), min(count, limit) — 8 B written per pattern
//       instead of 12; per tile (a search block's 2 x 256 patterns) the total, added by each
//       wave (locate_split_store, wave_tile_add).
//   (2) k_scan_chained: the exclusive scan of the tile totals, a block per 1024 tiles (C4:
//       24 k tiles); past kScanMaxBlocks kScanBlock tiles the one-block k_scan_tiles;
//   (3) k_locate_emit: per tile, the block's scan of its counts plus the tile's prefix
//       give the output offsets, then the positions straight from the records through SA;
//   (3') k_locate_walks, on walk-line indexes: the walks k_locate_emit listed;
//   then k_locate_emit_wide: the ranges over kLocSmall rows, a block per range.
// (A look-back inside the search kernel, measured in round 3, made every block wait for the
// slowest search among its predecessors: 3.2 ms against 1.1 ms; the other forms round 5
// tried are listed at k_locate_emit.)  Against the two phases this drops the scan of a
// 100-MB count array and the host round trip between the phases.
// Indexes without the full suffix array but with walk lines and text-position marks (C5;
// C4 under CS_FM_FULL_SA=0) take the same launches (round 3): a position is the
// short walk from its row (walk_position: at most pstride - 1 LF steps, one 32-B walk line
// each, then the mark's sample) instead of SA[row], in (1) for a pattern's only position
// and in (3) / k_locate_emit_wide for the rest (kPos: 0 the full SA, 1 WalkLine, 2
// WalkLineW).  Counts are u64 (cnt64) when the index is wide.
// The outputs (offsets and positions) leave through non-temporal stores (st_out).
#pragma once
#include "fm_walk.hpp"

namespace fmx {

struct OnePass {
  uint32_t* cnt = nullptr;               // (1) -> (3): min(count, limit) per pattern (narrow),
                                         // unless its record is a stashed position (count 1)
  uint64_t* cnt64 = nullptr;             // the same, wide indexes
  uint64_t* rec = nullptr;               // (1) -> (3): the pattern's record
  uint64_t* tiles = nullptr;             // per tile (a search block's patterns): its total, then
                                         // its exclusive prefix (k_scan_chained)
  const uint32_t* sa = nullptr;          // full suffix array
  uint64_t* out_offs = nullptr;          // npat + 1 exclusive offsets
  uint64_t* out_pos = nullptr;           // positions, `cap` of them
  uint64_t cap = 0;
  uint64_t* wide = nullptr;              // (q, first row) of ranges over kLocSmall rows
  unsigned long long* nwide = nullptr;
  uint64_t wide_cap = 0;
  uint32_t defer = 0;  // locate records: a pattern its record does not answer -> k_locate_list
  // walk-line indexes (kPos 1 / 2): the positions of patterns with 2..kLocSmall rows, as
  // (output index, row | adj << kWalkAdjShift) pairs for k_locate_walks — one lane per position, so no
  // emit wave waits on a lane's chain of walks — kLocTile slots per tile (tile t's at
  // t kLocTile, their number in wcnt[t]: no global counter); past them the emit walks them
  uint64_t* walks = nullptr;
  uint32_t* wcnt = nullptr;
  // k_scan_chained: per scan block its published total (bit 63: ready), zeroed by the search
  // kernel's block 0 (or a memset where no search kernel runs)
  unsigned long long* sflags = nullptr;
};

// The finish's host side (fm_locate.hip).
// The call's buffers: `lists` bytes for the caller's long-pattern lists first, then the parts
// of a LocateLayout (per pattern its record and count, the tiles, the wide ranges, on
// walk-line indexes the walk list, the chained scan's flags) — in the caller's workspace when
// it holds ws_lists + the layout's bytes (the workspace's lists sit where a count's do:
// ws_lists = count_workspace_bytes), else in one stream-ordered allocation (own).
// locate_buffers sets base, in_ws and op's pointers into the layout, op.sa and op.wide_cap;
// the outputs, the capacity and `defer` are the caller's to set.
struct LocateBufs {
  StreamBuf own;
  uint8_t* base = nullptr;  // the lists' place
  bool in_ws = false;
  OnePass op;
};
cs_status locate_buffers(const cs_fm_index* h, uint64_t npat, uint64_t wide_cap, uint64_t ws_lists,
                         uint64_t lists, const Work& work, hipStream_t st, LocateBufs& b);
// Stages (2), (3), (3') and the wide ranges after the search launches, the copy of the total
// (d_out_offs[npat]) to *total and the call's one synchronisation.  kpos as the kernels' kPos.
cs_status launch_locate_finish(const DevIndex& ix, uint64_t npat, uint64_t tiles, int kpos,
                               const OnePass& op, uint64_t* total, hipStream_t st);
// 4 blocks of 4 waves per CU of the current device (fm_query.hip, long_list_grid)
unsigned list_blocks_per_device();

namespace {

constexpr uint32_t kScanBlock = 1024;     // tiles per block of k_scan_chained
constexpr uint32_t kScanMaxBlocks = 1024; // (its look-back: one predecessor per thread)
__device__ __forceinline__ void onepass_zero(const OnePass& op) {
  // the call's wide-range counter and the chained scan's flags and ticket (no memset launch;
  // stream order makes the stores visible to the kernels after this one)
  if (threadIdx.x == 0) {
    if (blockIdx.x == 0) *op.nwide = 0;
    if (op.sflags && blockIdx.x < kScanMaxBlocks) op.sflags[blockIdx.x] = 0;
    if (op.sflags && blockIdx.x == 0) op.sflags[kScanMaxBlocks] = 0;
  }
}
// Tiles of the one-call locate's scan (k_count_ctx kOne with U = 2 patterns per lane)
constexpr uint64_t kLocTile = 2 * kBlk;
static_assert(kLocTile == kLongRegion, "a tile is a region: one block's patterns");

// position of BWT row `row` for the one-call locate: SA[row] (kPos 0) or the short walk
template <int kPos>
__device__ __forceinline__ uint64_t onepass_pos(const DevIndex& ix, const NodeTable& T, const OnePass& op,
                                                uint64_t row) {
  if constexpr (kPos == 0) return load_sa(op.sa, row);
  else return walk_position<WalkLineOf<kPos>>(ix, T, row);
}

// Exclusive scan over the block's U x kBlk values in pattern order (segment j holds the
// patterns q0 + j kBlk, j < U): mine[j] = the offset of the lane's j-th value inside the
// block, agg = the block's total.  Every thread of the block.
// (block_scan_excl's two halves around one barrier for the U segments, not U barriers)
template <int U>
__device__ __forceinline__ void block_scan(const uint64_t* kc, uint64_t* mine, uint64_t& agg) {
  constexpr int NW = kBlk / 64;
  __shared__ uint64_t s_wsum[U][NW];
  uint64_t x[U];
#pragma unroll
  for (int j = 0; j < U; ++j) {
    x[j] = kc[j];
    wave_scan_incl(x[j]);
    if ((threadIdx.x & 63) == 63) s_wsum[j][threadIdx.x >> 6] = x[j];
  }
  __syncthreads();
  agg = 0;
#pragma unroll
  for (int j = 0; j < U; ++j) {
    uint64_t before = agg;
    const int wv = threadIdx.x >> 6;
    for (int w2 = 0; w2 < NW; ++w2) {
      if (w2 < wv) before += s_wsum[j][w2];
      agg += s_wsum[j][w2];
    }
    mine[j] = before + x[j] - kc[j];
  }
}

__device__ __forceinline__ void tile_total_add(const OnePass& op, uint64_t tile, uint64_t v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(op.tiles + tile), v);
}

// Adds each lane's kc (0: nothing) to op.tiles[tile]: one atomic per distinct tile of the
// wave (a list launch's wave holds one or two slots' patterns, so one or two tiles; a
// pattern-per-lane atomic puts 512 same-address atomics on every tile: C4 150-mer locate
// 2.1 -> 3.4 ms).  Every lane of the wave, in uniform control flow.
__device__ __forceinline__ void wave_tile_add(const OnePass& op, uint64_t tile, uint64_t kc) {
  const uint32_t lane = threadIdx.x & 63;
  uint64_t pend = __ballot(kc != 0);
  while (pend) {
    const uint32_t l = (uint32_t)__ffsll((unsigned long long)pend) - 1u;
    const uint64_t t = __shfl(tile, (int)l, 64);
    const bool in = kc != 0 && tile == t;
    uint64_t s = in ? kc : 0;
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) s += __shfl_xor(s, dd, 64);
    if (lane == l) tile_total_add(op, t, s);
    pend &= ~__ballot(in);
  }
}

// (1)'s tail: the lane's results.
// A pattern reporting exactly one position gets it here, from the record already in the
// lane (its first row: SA[row] - k for a context window), so its SA read overlaps the
// other blocks' record reads instead of waiting for k_locate_emit; the record then holds
// kLocStash | position and stands for the count 1 (no count is stored: 8 B per pattern).
// (C4 Q_text: 99.6 % of the patterns.)
constexpr uint64_t kLocStash = 1ull << 62;  // with bit 63 clear: not a window, not a row
__device__ __forceinline__ bool loc_stashed(uint64_t r) { return (r >> 62) == 1; }
// skip: bit j set = the lane's j-th pattern is k_locate_long's (routing): its count and record
// are left for that kernel to write
// kWaveTile (the barrier-free search, kPos 0): each wave adds its patterns' total to the tile
// (zeroed at the block's start) instead of a block scan storing it, so no wave waits for the
// block's others
template <int U, int kPos = 0, bool kWaveTile = false>
__device__ __forceinline__ void locate_split_store(const DevIndex& ix, const NodeTable& T, uint64_t npat,
                                                   uint64_t tile, uint64_t q0, const uint64_t* kc,
                                                   const uint64_t* kr, const OnePass& op, uint32_t skip = 0) {
  const uint64_t n = ix.n;
  uint64_t rs[U];
  if constexpr (kWaveTile) {
    uint64_t sum = 0;
#pragma unroll
    for (int j = 0; j < U; ++j) sum += kc[j];
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) sum += __shfl_xor(sum, dd, 64);
    if ((threadIdx.x & 63) == 0 && sum) tile_total_add(op, tile, sum);
  } else {
    uint64_t mine[U], agg;
    block_scan<U>(kc, mine, agg);
    if (threadIdx.x == 0) op.tiles[tile] = agg;
  }
  uint64_t row[U], adj[U];
  bool one[U];
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const uint64_t q = q0 + (uint64_t)j * kBlk, s = kr[j];
    rs[j] = s;
    row[j] = s;
    adj[j] = 0;
    one[j] = q < npat && kc[j] == 1 && !loc_stashed(s);  // (not stashed by a locate record)
    uint32_t rel;
    if (one[j] && (s & kLocCtx)) loc_window(s, row[j], adj[j], rel);  // a window's only match: its first row
  }
  if constexpr (kPos == 0) {
#pragma unroll
    for (int j = 0; j < U; ++j)
      if (one[j]) row[j] = load_sa(op.sa, row[j]);
  } else {  // the lane's walks in lockstep: row[j] becomes the position
    bool act[U];
#pragma unroll
    for (int j = 0; j < U; ++j) act[j] = one[j];
    if constexpr (kWaveTile)  // (T is the global table: the walks' constants in registers)
      walk_positions_k<WalkLineOf<kPos>, U>(ix, T, walk_consts(T), row, act);
    else
      walk_positions<WalkLineOf<kPos>, U>(ix, T, row, act);
  }
#pragma unroll
  for (int j = 0; j < U; ++j)
    if (one[j]) rs[j] = kLocStash | pos_back(row[j], adj[j], n);
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const uint64_t q = q0 + (uint64_t)j * kBlk;
    if (q >= npat || ((skip >> j) & 1u)) continue;
    if (!(kc[j] == 1 && loc_stashed(rs[j]))) {  // the count, and no stash standing for 1
      if (op.cnt64) op.cnt64[q] = kc[j];
      else op.cnt[q] = (uint32_t)kc[j];
      if (loc_stashed(rs[j])) rs[j] = 0;  // (a limit of 0)
    }
    op.rec[q] = rs[j];
  }
}

}  // namespace
}  // namespace fmx

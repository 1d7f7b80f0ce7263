// fm_seeded.hip — seeded locate within k <= CS_SEED_MAX_K mismatches
// (cs_fmindex_approx_seeded.h): the pattern's k + 1 pigeonhole pieces located exactly by the
// two-phase locate (launch_locate_ranges, launch_locate_walk: the pieces tile the patterns, so
// they are patterns of the same buffer under a refined offsets array), every hit verified
// against the byte text in HBM (k_seed_verify, the hot path), the accepted candidates
// compacted by one scan.  A candidate is one hit of one piece; a pattern's candidates are one
// contiguous segment of the candidate arrays, pieces ascending, so the global scan is the
// per-pattern compaction and its order is the output's.
#include <rocprim/iterator/transform_iterator.hpp>

#include "fm_search.hpp"

namespace fmx {
namespace {

constexpr uint8_t kSeedReject = 0xFF;  // res[c] of a candidate that is not emitted

// Piece offsets: poffs[q (k + 1) + p] = o0 + floor(p m / (k + 1)) for pattern q = [o0, o0 + m),
// poffs[npat (k + 1)] = the batch's end (offs == nullptr: patterns of fixed_m bytes back to
// back).  short_q (preset to all ones): the smallest q with 0 < m <= k.  p m stays below 2^64
// for any pattern that fits a device (p <= 15).
__global__ __launch_bounds__(kBlk) void k_seed_pieces(const uint64_t* __restrict__ offs, uint64_t fixed_m,
                                                      uint64_t npat, uint32_t k,
                                                      uint64_t* __restrict__ poffs,
                                                      unsigned long long* short_q) {
  const uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x, np = npat * (k + 1);
  if (e > np) return;
  if (e == np) {
    poffs[e] = offs ? offs[npat] : npat * fixed_m;
    return;
  }
  const uint64_t q = e / (k + 1), p = e - q * (k + 1);
  const uint64_t o0 = offs ? offs[q] : q * fixed_m, m = offs ? offs[q + 1] - o0 : fixed_m;
  poffs[e] = o0 + p * m / (k + 1);
  if (p == 0 && m != 0 && m <= k) atomicMin(short_q, (unsigned long long)q);
}

// 16 bytes as two little-endian words: byte i of the vector is byte i & 7 of w[i >> 3]
struct V16 {
  uint64_t lo, hi;
};

// The 16-B aligned vector at address w, of which only bytes inside [lo, hi) may be touched: one
// vector load when it lies inside, else its bytes inside one by one (the others read as zero).
__device__ __forceinline__ V16 load16_in(uintptr_t w, uintptr_t lo, uintptr_t hi) {
  V16 v{0, 0};
  if (w >= lo && w + 16 <= hi && w + 16 > w) {
    const uint4 x = *reinterpret_cast<const uint4*>(w);
    v.lo = ((uint64_t)x.y << 32) | x.x;
    v.hi = ((uint64_t)x.w << 32) | x.z;
    return v;
  }
#pragma unroll
  for (uint32_t i = 0; i < 16; ++i) {
    const uintptr_t a = w + i;
    if (a >= lo && a < hi && a >= w) {
      const uint64_t b = *reinterpret_cast<const uint8_t*>(a);
      if (i < 8) v.lo |= b << (8 * i);
      else v.hi |= b << (8 * (i - 8));
    }
  }
  return v;
}

__device__ __forceinline__ uint64_t funnel8(uint64_t a, uint64_t b, uint32_t bits) {
  return bits ? (a >> bits) | (b << (64 - bits)) : a;
}

// bytes [sh, sh + 16) of the 32 bytes a ++ b, sh < 16
__device__ __forceinline__ V16 shift16(const V16& a, const V16& b, uint32_t sh) {
  const bool up = sh >= 8;
  const uint64_t x0 = up ? a.hi : a.lo, x1 = up ? b.lo : a.hi, x2 = up ? b.hi : b.lo;
  const uint32_t bits = (sh & 7) * 8;
  return V16{funnel8(x0, x1, bits), funnel8(x1, x2, bits)};
}

// the bytes [a, b) of a word kept (0 <= a <= b <= 8)
__device__ __forceinline__ uint64_t byte_mask(uint32_t a, uint32_t b) {
  const uint64_t below_b = b >= 8 ? ~0ull : (1ull << (8 * b)) - 1;
  const uint64_t below_a = a >= 8 ? ~0ull : (1ull << (8 * a)) - 1;
  return below_b & ~below_a;
}

// the number of non-zero bytes of x
__device__ __forceinline__ uint32_t nonzero_bytes(uint64_t x) {
  constexpr uint64_t k7f = 0x7F7F7F7F7F7F7F7Full;
  return (uint32_t)__popcll((((x & k7f) + k7f) | x) & ~k7f);
}

// The mismatching bytes of P[a, b) against the window at text position s, for a window that
// does not wrap (s + m <= n): the 16-B aligned text vectors holding a byte of
// text[s + a, s + b), each against the pattern's bytes at the same window offsets — two aligned
// pattern vectors shifted by the difference of the two misalignments, the second carried to
// the next step — under the byte mask of the piece's edges.  Alignment is taken from the
// address values (the caller's d_pats may be odd).  [tlo, thi) is the text, [plo, phi) the
// batch's pattern bytes: no load touches a byte outside them.
__device__ __forceinline__ uint32_t piece_diff(uintptr_t ta, uintptr_t pa, uint64_t a, uint64_t b,
                                               uintptr_t tlo, uintptr_t thi, uintptr_t plo, uintptr_t phi) {
  const uintptr_t t0 = ta + a, t1 = ta + b;  // the piece's text bytes [t0, t1)
  const uintptr_t first = t0 & ~(uintptr_t)15, last = (t1 - 1) & ~(uintptr_t)15;
  uint32_t cnt = 0;
  V16 carry{0, 0};
  uintptr_t carry_at = 0;  // the pattern vector the previous step loaded last
  for (uintptr_t w = first; w <= last && w >= first; w += 16) {
    const V16 t = load16_in(w, tlo, thi);
    const uintptr_t pw = pa + (w - ta);  // the pattern address facing text address w (wraps below pa)
    const uintptr_t pv = pw & ~(uintptr_t)15;
    const uint32_t sh = (uint32_t)(pw & 15);
    const V16 p0 = (carry_at == pv && w != first) ? carry : load16_in(pv, plo, phi);
    const V16 p1 = sh ? load16_in(pv + 16, plo, phi) : V16{0, 0};
    carry = sh ? p1 : p0;
    carry_at = sh ? pv + 16 : pv;
    const V16 p = shift16(p0, p1, sh);
    // bytes [i0, i1) of this vector belong to the piece
    const uint32_t i0 = w < t0 ? (uint32_t)(t0 - w) : 0u, i1 = t1 - w < 16 ? (uint32_t)(t1 - w) : 16u;
    const uint64_t mlo = byte_mask(i0 < 8 ? i0 : 8, i1 < 8 ? i1 : 8);
    const uint64_t mhi = byte_mask(i0 > 8 ? i0 - 8 : 0, i1 > 8 ? i1 - 8 : 0);
    cnt += nonzero_bytes((t.lo ^ p.lo) & mlo) + nonzero_bytes((t.hi ^ p.hi) & mhi);
  }
  return cnt;
}

// the same for any window, byte by byte with the modulo (windows through the end of the text,
// patterns longer than the text)
__device__ __forceinline__ uint32_t piece_diff_cyclic(const uint8_t* __restrict__ text, uint64_t n,
                                                      const uint8_t* __restrict__ P, uint64_t s, uint64_t a,
                                                      uint64_t b) {
  uint32_t cnt = 0;
  for (uint64_t j = a; j < b; ++j) cnt += text[(s + j % n) % n] != P[j];
  return cnt;
}

// Verification, the hot path: candidate c (one per lane) is hit c of the
// piece list — its piece j by an upper-bound search in cand_offs (at most 64 halvings), its
// pattern q = j / (k + 1), p = j mod (k + 1), its alignment s = (pos - a_p) mod n.  The pieces
// p' = 0..k in order, each counted against the text window at s: a clean piece p' < p owns the
// alignment (reject), a running sum past k rejects, piece p itself is known clean and not
// read.  res[c] = the distance, or kSeedReject; cand_pos[c] = s.  Every loop is bounded by
// construction (the search by log2, the compares by m) and nothing waits on another wave.
// (A form with eight lanes per candidate, 128 contiguous window bytes per step and the counts
// combined by shuffles, lost to this one at every length measured and was deleted: DESIGN §10.8.)
__global__ __launch_bounds__(kBlk) void k_seed_verify(const uint8_t* __restrict__ text, uint64_t n,
                                                      const uint8_t* __restrict__ pats,
                                                      const uint64_t* __restrict__ poffs,
                                                      const uint64_t* __restrict__ cand_offs,
                                                      uint64_t npieces, uint32_t k, uint64_t ncand,
                                                      uint64_t* __restrict__ cand_pos,
                                                      uint8_t* __restrict__ res) {
  const uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (c >= ncand) return;
  uint64_t lo = 0, hi = npieces;  // the first piece whose end is past c
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (cand_offs[mid + 1] <= c) lo = mid + 1;
    else hi = mid;
  }
  const uint64_t j = lo, q = j / (k + 1);
  const uint32_t p = (uint32_t)(j - q * (k + 1));
  const uint64_t* const po = poffs + q * (k + 1);
  const uint64_t o0 = po[0], m = po[k + 1] - o0;
  const uint64_t ap = po[p] - o0;
  const uint64_t s = (cand_pos[c] + n - ap % n) % n;
  const bool wraps = s + m > n || s + m < s;
  const uintptr_t tlo = reinterpret_cast<uintptr_t>(text), thi = tlo + n;
  const uintptr_t plo = reinterpret_cast<uintptr_t>(pats) + poffs[0];
  const uintptr_t phi = reinterpret_cast<uintptr_t>(pats) + poffs[npieces];
  uint32_t d = 0;
  bool keep = true;
  uint64_t a = 0;
  for (uint32_t pp = 0; pp <= k && keep; ++pp) {
    const uint64_t b = po[pp + 1] - o0;
    if (pp != p) {
      const uint32_t x = wraps ? piece_diff_cyclic(text, n, pats + o0, s, a, b)
                               : piece_diff(tlo + s, reinterpret_cast<uintptr_t>(pats) + o0, a, b, tlo, thi,
                                            plo, phi);
      d += x;
      keep = !(pp < p && x == 0) && d <= k;
    }
    a = b;
  }
  res[c] = keep ? (uint8_t)d : kSeedReject;
  cand_pos[c] = s;
}

// d_out_offs[q] = slot[cand_offs[q (k + 1)]] — the accepted candidates before pattern q's
// first — and d_out_offs[npat] = slot[ncand], the total
__global__ __launch_bounds__(kBlk) void k_seed_offs(const uint64_t* __restrict__ slot,
                                                    const uint64_t* __restrict__ cand_offs, uint64_t npat,
                                                    uint32_t k, uint64_t* __restrict__ out_offs) {
  const uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (q <= npat) out_offs[q] = slot[cand_offs[q * (k + 1)]];
}

__global__ __launch_bounds__(kBlk) void k_seed_emit(const uint64_t* __restrict__ slot,
                                                    const uint64_t* __restrict__ cand_pos,
                                                    const uint8_t* __restrict__ res, uint64_t ncand,
                                                    uint64_t* __restrict__ out_pos,
                                                    uint8_t* __restrict__ out_dist) {
  const uint64_t c = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (c >= ncand) return;
  const uint8_t d = res[c];
  if (d == kSeedReject) return;
  const uint64_t o = slot[c];
  out_pos[o] = cand_pos[c];
  out_dist[o] = d;
}

struct SeedAccepted {
  __device__ __forceinline__ uint64_t operator()(uint8_t r) const { return r != kSeedReject ? 1u : 0u; }
};

// a candidate-sized temporary: CS_ERR_OOM names the candidate count
cs_status seed_alloc(StreamBuf& b, uint64_t bytes, uint64_t ncand, hipStream_t st) {
  const hipError_t e = b.alloc(bytes, st);
  if (e == hipSuccess) return CS_OK;
  const cs_status s = hip_fail(e, "hipMallocAsync (seeded locate candidates)");
  if (s == CS_ERR_OOM)
    set_error("seeded locate: no memory for " + std::to_string(ncand) + " candidates (about 17 bytes each)");
  return s;
}

}  // namespace

cs_status launch_seed_search(const cs_fm_index* h, const uint8_t* d_pats, const uint64_t* d_offs,
                             uint64_t npat, uint32_t k, uint64_t fixed_m, uint32_t flags, hipStream_t st,
                             SeedPlan& plan, hipEvent_t* ev) {
  const uint64_t np = npat * (k + 1);
  plan.npieces = np;
  StreamBuf ctl;  // [0] the first pattern with 0 < m <= k, or all ones
  FMX_HIP(plan.poffs.alloc((np + 1) * 8, st));
  FMX_HIP(plan.sp.alloc((np ? np : 1) * 8, st));
  FMX_HIP(plan.cand_offs.alloc((np + 1) * 8, st));
  FMX_HIP(ctl.alloc(8, st));
  FMX_HIP(hipMemsetAsync(ctl.p, 0xFF, 8, st));
  if (ev) FMX_HIP(hipEventRecord(ev[0], st));
  k_seed_pieces<<<grid_for(np + 1, kBlk, 0xFFFFFFFFu), kBlk, 0, st>>>(
      d_offs, fixed_m, npat, k, plan.poffs.as<uint64_t>(), ctl.as<unsigned long long>());
  FMX_HIP(hipGetLastError());
  // read back with the candidate total (launch_locate_ranges synchronises st); should that call
  // fail before it synchronises, the copy into this frame is waited for before the frame goes
  uint64_t short_q = ~0ull;
  FMX_HIP(hipMemcpyAsync(&short_q, ctl.p, 8, hipMemcpyDeviceToHost, st));
  cs_status s = launch_locate_ranges(h, d_pats, plan.poffs.as<uint64_t>(), np, /*limit*/ h->n,
                                     plan.sp.as<uint64_t>(), plan.cand_offs.as<uint64_t>(), &plan.ncand, st,
                                     flags);
  if (s != CS_OK) {
    (void)hipStreamSynchronize(st);
    return s;
  }
  if (ev) FMX_HIP(hipEventRecord(ev[1], st));
  if (short_q != ~0ull) {
    set_error("seeded locate: pattern " + std::to_string(short_q) + " is not longer than k = " +
              std::to_string(k));
    return CS_ERR_INVALID;
  }
  return CS_OK;
}

cs_status launch_seed_verify(const cs_fm_index* h, const uint8_t* d_pats, uint64_t npat, uint32_t k,
                             uint64_t* d_out_offs, uint32_t flags, hipStream_t st, SeedPlan& plan,
                             hipEvent_t* ev) {
  const uint64_t C = plan.ncand;
  if (!C) {  // no candidate: every pattern's segment is empty
    plan.total = 0;
    FMX_HIP(hipMemsetAsync(d_out_offs, 0, (npat + 1) * 8, st));
    if (ev)
      for (int i = 2; i <= 4; ++i) FMX_HIP(hipEventRecord(ev[i], st));
    FMX_HIP(hipStreamSynchronize(st));
    return CS_OK;
  }
  StreamBuf err, tmp;
  cs_status s;
  if ((s = seed_alloc(plan.cand_pos, C * 8, C, st)) != CS_OK) return s;
  if ((s = seed_alloc(plan.res, C + 1, C, st)) != CS_OK) return s;
  if ((s = seed_alloc(plan.slot, (C + 1) * 8, C, st)) != CS_OK) return s;
  FMX_HIP(err.alloc(8, st));
  FMX_HIP(hipMemsetAsync(err.p, 0xFF, 8, st));
  // the positions of the pieces' hits: the exact locate's phase 2 with the pieces as its patterns
  s = launch_locate_walk(h, plan.sp.as<uint64_t>(), plan.cand_offs.as<uint64_t>(), plan.npieces, C,
                         plan.cand_pos.as<uint64_t>(), st, err.as<unsigned long long>(), flags);
  if (s != CS_OK) return s;
  if (ev) FMX_HIP(hipEventRecord(ev[2], st));
  k_seed_verify<<<grid_for(C, kBlk, 0xFFFFFFFFu), kBlk, 0, st>>>(
      static_cast<const uint8_t*>(h->d_dtext), h->n, d_pats, plan.poffs.as<uint64_t>(),
      plan.cand_offs.as<uint64_t>(), plan.npieces, k, C, plan.cand_pos.as<uint64_t>(), plan.res.as<uint8_t>());
  FMX_HIP(hipGetLastError());
  FMX_HIP(hipMemsetAsync(plan.res.as<uint8_t>() + C, kSeedReject, 1, st));  // the scan's slot for the total
  if (ev) FMX_HIP(hipEventRecord(ev[3], st));
  auto in = rocprim::make_transform_iterator(plan.res.as<uint8_t>(), SeedAccepted{});
  size_t tb = 0;
  FMX_HIP(rocprim::exclusive_scan(nullptr, tb, in, plan.slot.as<uint64_t>(), (uint64_t)0, C + 1,
                                  rocprim::plus<uint64_t>(), st));
  FMX_HIP(tmp.alloc(tb, st));
  FMX_HIP(rocprim::exclusive_scan(tmp.p, tb, in, plan.slot.as<uint64_t>(), (uint64_t)0, C + 1,
                                  rocprim::plus<uint64_t>(), st));
  k_seed_offs<<<grid_for(npat + 1, kBlk, 0xFFFFFFFFu), kBlk, 0, st>>>(
      plan.slot.as<uint64_t>(), plan.cand_offs.as<uint64_t>(), npat, k, d_out_offs);
  FMX_HIP(hipGetLastError());
  if (ev) FMX_HIP(hipEventRecord(ev[4], st));
  uint64_t bad = ~0ull;  // (nothing that can fail stands between a copy into this frame and the wait)
  FMX_HIP(hipMemcpyAsync(&plan.total, plan.slot.as<uint64_t>() + C, 8, hipMemcpyDeviceToHost, st));
  const hipError_t copied = hipMemcpyAsync(&bad, err.p, 8, hipMemcpyDeviceToHost, st);
  FMX_HIP(hipStreamSynchronize(st));
  FMX_HIP(copied);
  if (bad != ~0ull) {
    set_error("locate: LF walk exceeded text length");  // as check_locate_error reports it
    return CS_ERR_LF_OVERRUN;
  }
  return CS_OK;
}

cs_status launch_seed_emit(const SeedPlan& plan, uint64_t* d_out_pos, uint8_t* d_out_dist, hipStream_t st,
                           hipEvent_t* ev) {
  k_seed_emit<<<grid_for(plan.ncand, kBlk, 0xFFFFFFFFu), kBlk, 0, st>>>(
      plan.slot.as<uint64_t>(), plan.cand_pos.as<uint64_t>(), plan.res.as<uint8_t>(), plan.ncand, d_out_pos,
      d_out_dist);
  FMX_HIP(hipGetLastError());
  if (ev) FMX_HIP(hipEventRecord(ev[5], st));
  return CS_OK;
}

}  // namespace fmx

// G1 MSM engine, steps 1-3 of the pipeline (msm.hip has the overview): the launch's pointer tables, the three sorting fronts
// that turn scalars (or bucket numbers) into per-bucket entry lists -- plain digits + scatter, the two/three-pass partition
// sort of the table launches, the index front of the bucket-sum launches.  The plan scans between a front's counting and
// placing halves are msm_plan (msm_plan.hip).  One host function per front enqueues it (msm_front_*), on the buffers of an MsmBuffers view.
#include <algorithm>
#include "msm.hpp"
#include "msm_device.hpp"
#include "curve29.hpp"

namespace cq {

// ---- pointer tables (per-MSM scalar / base arrays), written from a by-value kernel argument ------
// `ln`: the length the SORT sees (0 for an MSM whose entry lists are another MSM's, see msm_run); `src`: the MSM whose
// lists an MSM accumulates from (itself, unless it shares its scalars with an earlier one)
// The launch's first kernel: the pointer / length tables the later kernels read, and the counts and sort cursors cleared
// (16-byte stores, grid-stride) -- one launch instead of a 5 us kernel and a 5 us memset at the head of every front.
__global__ __launch_bounds__(256) void msm_set_ptrs_kernel(MsmPtrs sc, MsmPtrs bs, MsmStrides st, MsmStrides ln, MsmStrides src, const void** dst,
                                                          uint32_t batch, uint4* __restrict__ zero, size_t zero_quads) {
  CQ_CRITICAL_WAVES();
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < zero_quads; i += (size_t)gridDim.x * blockDim.x)
    zero[i] = make_uint4(0, 0, 0, 0);
  if (blockIdx.x) return;
  const uint32_t t = threadIdx.x;
  if (t < batch) {
    dst[t] = sc.p[t];
    dst[batch + t] = bs.p[t];
    ((uint64_t*)(dst + 2 * batch))[t] = st.s[t];
    ((uint64_t*)(dst + 3 * batch))[t] = ln.s[t];
    ((uint64_t*)(dst + 4 * batch))[t] = src.s[t];
  }
}

// ---- 1. digits + histogram -------------------------------------------------------------------
// signed c-bit digit of window w of the canonical scalar v, with the running carry
static __device__ __forceinline__ uint32_t signed_digit(const U256& v, uint32_t w, uint32_t c, uint32_t& carry, uint32_t& neg) {
  const uint32_t M = 1u << (c - 1);
  const uint32_t bitpos = w * c;
  const uint32_t word = bitpos >> 5, sh = bitpos & 31;
  uint32_t raw = 0;
  if (word < 8) {
    uint64_t two = v.l[word];
    if (word + 1 < 8) two |= (uint64_t)v.l[word + 1] << 32;
    raw = (uint32_t)(two >> sh) & ((1u << c) - 1);
  }
  uint32_t d = raw + carry;
  neg = 0;
  carry = 0;
  if (d > M) {
    d = (1u << c) - d;
    neg = 1;
    carry = 1;
  }
  return d;
}

// One lane per scalar: every window's digit bumps the histogram; the value the atomic returns is the
// entry's rank inside its bucket, kept for the scatter pass (so the sort needs one atomic per entry).
//
// The kernel is bound by atomic round trips, so a wave never waits for one before issuing the next: windows are
// handled DIGIT_GROUP at a time -- all their atomics go out back to back (one instruction per window), and only
// then are the returned values turned into ranks.  Within a window the lanes that share the key of the first
// two pending lanes (hot keys: 0/1 columns, sparse top windows) are folded into their leader's atomic, which
// adds the group size; `meta` remembers leader lane and position inside the group.
constexpr uint32_t DIGIT_GROUP = 6;
__global__ __launch_bounds__(256) void msm_digits_kernel(const Fr* const* __restrict__ scalars, const uint64_t* __restrict__ lens,
                                                         uint32_t nmax, uint32_t c, uint32_t nwin, uint32_t pre,
                                                         uint32_t* __restrict__ ranks, uint32_t* __restrict__ counts) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t m = blockIdx.y;
  const uint32_t lane = threadIdx.x & 63;
  const bool live = i < (uint32_t)lens[m];
  U256 v;
  if (live) v = scalars[m][i].to_canonical();
  else for (int k = 0; k < 8; k++) v.l[k] = 0;
  const uint32_t M = 1u << (c - 1);
  uint32_t carry = 0, neg;
  for (uint32_t w0 = 0; w0 < nwin; w0 += DIGIT_GROUP) {
    uint32_t ret[DIGIT_GROUP], meta[DIGIT_GROUP];  // meta: 0xffffffff = inactive, else leader lane << 8 | offset, leader 64 = none
#pragma unroll
    for (uint32_t q = 0; q < DIGIT_GROUP; q++) {
      const uint32_t w = w0 + q;
      meta[q] = 0xffffffffu;
      ret[q] = 0;
      if (w >= nwin) continue;  // wave-uniform
      const uint32_t d = signed_digit(v, w, c, carry, neg);
      const size_t mw = (size_t)m * nwin + w;
      // precomputed-table mode folds every window into one bucket set per MSM
      const bool act = live && d != 0;
      const uint32_t key = (uint32_t)((pre ? (size_t)m : mw) * M) + (d - 1);
      bool pending = act;
      uint32_t add = 1, lead = 64, below = 0;
      bool issue = act;
#pragma unroll
      for (int round = 0; round < 2; round++) {
        const unsigned long long pend = __ballot(pending);
        if (pend) {  // wave-uniform
          const int leader = __ffsll((long long)pend) - 1;
          const uint32_t lkey = __shfl(key, leader, 64);
          const bool mine = pending && key == lkey;
          const unsigned long long grp = __ballot(mine);
          if (mine) {
            lead = (uint32_t)leader;
            below = __popcll(grp & ((1ull << lane) - 1ull));
            add = __popcll(grp);
            issue = (int)lane == leader;
            pending = false;
          }
        }
      }
      if (issue) ret[q] = atomicAdd(&counts[key], (lead == lane || lead == 64) ? add : 1u);
      if (act) meta[q] = (lead << 8) | below;
    }
#pragma unroll
    for (uint32_t q = 0; q < DIGIT_GROUP; q++) {
      const uint32_t w = w0 + q;
      if (w >= nwin) continue;
      const uint32_t lead = (meta[q] >> 8) & 0xff;
      const uint32_t base = __shfl(ret[q], lead & 63, 64);  // every lane takes part in the shuffle
      if (meta[q] != 0xffffffffu) {
        const uint32_t rank = lead < 64 ? base + (meta[q] & 0xff) : ret[q];
        ranks[((size_t)m * nwin + w) * nmax + i] = rank;
      }
    }
  }
}

// Precomputed-table mode (one bucket set of M = 2^14 buckets per MSM): a two-pass (MSD) counting sort.
//
// A single-pass sort drops every 4-byte entry at a random place of its MSM's list array; the L2 evicts those as
// 32-byte partial writes (measured: 32 B of write traffic per entry, 1.3 TB/s, twice that only while a whole launch
// fits the 256 MB memory-side cache), and the per-entry rank array costs another 8 B.  Here every pass writes runs:
//   a. part_hist    : per chunk of 2048 scalars, LDS histogram of the entries' PARTITION (bucket >> 7: 128
//                     partitions of 128 buckets per MSM); one device atomic per (chunk, partition).
//   b. part_scan    : exclusive scan of the partition sizes (<= 32 x 128 values, one block).
//   c. part_scatter : same chunks; each reserves its range in every partition with one device atomic and writes its
//                     entries there as runs -- 4-byte payloads and, in a byte array of their own, the bucket inside the
//                     partition (5 bytes per entry; the counting pass then reads one byte per entry).
//   d. bucket_count : per partition, LDS histogram of its 128 buckets -> the global bucket counts (the plan's input).
//   e. bucket_place : after the plan: per tile of 4096 entries of a partition, LDS histogram, one device atomic
//                     per non-empty bucket to reserve the tile's run inside the bucket's list, entries written
//                     there (runs of ~32 entries).  PART_SPLIT workgroups share a partition tile by tile.
// d and e are part_count and part_tile_place with the BucketBins policy; the refinement pass of the wide windows (c > 17)
// is the same two bodies with RefineBins.
#ifndef CQ_PART_CHUNK_THREADS
#define CQ_PART_CHUNK_THREADS 256
#endif
constexpr uint32_t DIGITS_LDS_THREADS = CQ_PART_CHUNK_THREADS;
constexpr uint32_t DIGITS_LDS_PER_LANE = 8;
constexpr uint32_t DIGITS_LDS_CHUNK = DIGITS_LDS_THREADS * DIGITS_LDS_PER_LANE;
// (DIGITS_LDS_MAX_M, PART_BITS / PART_BUCKETS, PART_BITS_WIDE, PSC_MAX_WIN and part_shift_of: msm_layout.hpp, which sizes by them)
constexpr uint32_t PART_MAX = 256;                                 // partitions per MSM (128 up to c = 16, 256 for c = 17)
constexpr uint32_t PART_THREADS = 256, PART_PER_LANE = 16, PART_TILE = PART_THREADS * PART_PER_LANE;
constexpr uint32_t PART_SPLIT = 8;  // workgroups per partition in the bucket passes
static_assert(PART_MAX <= DIGITS_LDS_THREADS && (1u << PART_BITS_WIDE) <= PART_THREADS, "one thread per histogram bin");

// CW != 0: the window width and count are compile-time constants (the tables' c = 15, 17 windows): the digit loop unrolls,
// every limb index of the canonical scalar is an immediate (with a run-time window index the limbs sat in scratch memory)
template <uint32_t CW, uint32_t NW>
__global__ __launch_bounds__(DIGITS_LDS_THREADS) void msm_part_hist_kernel(const Fr* const* __restrict__ scalars,
                                                                           const uint64_t* __restrict__ lens, uint32_t c_, uint32_t nwin_,
                                                                           uint32_t npart, uint32_t per_lane, uint32_t* __restrict__ psize) {
  CQ_CRITICAL_WAVES();
  __shared__ uint32_t hist[PART_MAX];
  const uint32_t c = CW ? CW : c_, nwin = CW ? NW : nwin_;
  const uint32_t shift = part_shift_of(c);
  const uint32_t m = blockIdx.y, t = threadIdx.x;
  const uint32_t len = (uint32_t)lens[m];
  const uint32_t base = blockIdx.x * DIGITS_LDS_THREADS * per_lane;
  if (base >= len) return;  // block-uniform
  if (t < npart) hist[t] = 0;
  __syncthreads();
  for (uint32_t k = 0; k < per_lane; k++) {
    const uint32_t i = base + k * DIGITS_LDS_THREADS + t;
    if (i >= len) continue;
    const U256 v = scalars[m][i].to_canonical();
    uint32_t carry = 0, neg;
#pragma unroll
    for (uint32_t w = 0; w < (CW ? NW : 32u); w++) {
      if (!CW && w >= nwin) break;
      const uint32_t d = signed_digit(v, w, c, carry, neg);
      if (d) atomicAdd(&hist[(d - 1) >> shift], 1u);
    }
  }
  __syncthreads();
  if (t < npart && hist[t]) atomicAdd(&psize[m * npart + t], hist[t]);
}

// exclusive scan of P <= 4096 values in one block: poff[0..P], poff[P] = total
// `s1_out` (first pass only): the sub-list length of the accumulate level for THIS launch's entries -- the host picks it from
// the bound batch x windows x n, but a launch of sparse or small scalars (advice columns of 24-bit limbs on a tenth of the
// rows, multiplicities) has a fiftieth of that, and its accumulate kernel is then a chain of s1 dependent additions on a
// fraction of the SIMDs: msm_small_launch_s1 of the entries actually there (an MSM that reads another one's lists counts
// with that one's), never more than the host's value.
__global__ __launch_bounds__(1024) void msm_part_scan_kernel(const uint32_t* __restrict__ psize, uint32_t P, uint32_t* __restrict__ poff,
                                                             const uint64_t* __restrict__ list_src = nullptr, uint32_t batch = 0,
                                                             uint32_t npart = 0, uint32_t s1_host = 0, uint32_t* __restrict__ s1_out = nullptr) {
  CQ_CRITICAL_WAVES();
  __shared__ uint32_t part[1024];
  const uint32_t per = (P + 1023) / 1024;
  const uint32_t lo = min(threadIdx.x * per, P), hi = min(lo + per, P);
  uint32_t s = 0;
  for (uint32_t j = lo; j < hi; j++) s += psize[j];
  part[threadIdx.x] = s;
  __syncthreads();
  for (uint32_t off = 1; off < 1024; off <<= 1) {
    const uint32_t v = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  uint32_t run = part[threadIdx.x] - s;
  for (uint32_t j = lo; j < hi; j++) {
    poff[j] = run;
    run += psize[j];
  }
  if (threadIdx.x == 1023) poff[P] = part[1023];
  if (s1_out) {
    __syncthreads();  // poff is complete (this block wrote all of it)
    if (threadIdx.x == 0) {
      uint64_t entries = 0;
      for (uint32_t m = 0; m < batch; m++) {
        const uint32_t src = (uint32_t)list_src[m];
        entries += poff[(src + 1) * npart] - poff[src * npart];
      }
      const uint32_t s1 = msm_small_launch_s1(entries);  // (the host's value stands for a launch that is not small)
      *s1_out = entries < (uint64_t)MSM_S1 * MSM_SMALL_LANES && s1 < s1_host ? s1 : s1_host;
    }
  }
}

// One scalar per lane; the chunk's entries are sorted by partition in LDS first, so that the write-out is a linear
// copy of runs (~34 entries = 272 B per partition) instead of one uncoalesced 8-byte store per entry (which kept the
// per-CU memory pipeline, not HBM, busy for 0.5 ms on a 21-MSM launch).
constexpr uint32_t PSC_THREADS = 256;
// LowT: the bucket inside the partition -- a byte up to c = 15 (7 bits), 16 bits for the wider windows (c - 8 bits)
template <uint32_t CW, uint32_t NW, typename LowT>
__global__ __launch_bounds__(PSC_THREADS) void msm_part_scatter_kernel(const Fr* const* __restrict__ scalars,
                                                                       const uint64_t* __restrict__ lens, uint32_t c_, uint32_t nwin_,
                                                                       uint32_t npart, const uint32_t* __restrict__ poff,
                                                                       uint32_t* __restrict__ pcursor, uint32_t* __restrict__ part_pay,
                                                                       LowT* __restrict__ part_low) {
  CQ_CRITICAL_WAVES();
  __shared__ uint2 stage[PSC_THREADS * (CW ? NW : PSC_MAX_WIN)];
  __shared__ uint32_t hist[PART_MAX], lstart[PART_MAX], gbase[PART_MAX];
  const uint32_t c = CW ? CW : c_, nwin = CW ? NW : nwin_;
  const uint32_t shift = part_shift_of(c);
  const uint32_t m = blockIdx.y, t = threadIdx.x;
  const uint32_t len = (uint32_t)lens[m];
  const uint32_t i = blockIdx.x * PSC_THREADS + t;
  if (blockIdx.x * PSC_THREADS >= len) return;  // block-uniform
  if (t < PART_MAX) hist[t] = 0;
  U256 v;
  if (i < len) v = scalars[m][i].to_canonical();
  else for (int q = 0; q < 8; q++) v.l[q] = 0;  // zero scalar: no non-zero digit
  __syncthreads();
  // the digits once, kept for the placement below: |digit| - 1 in the low half, the sign in bit 31, 0xffffffff = zero digit
  uint32_t dg[CW ? NW : PSC_MAX_WIN];
  {
    uint32_t carry = 0, neg;
#pragma unroll
    for (uint32_t w = 0; w < (CW ? NW : PSC_MAX_WIN); w++) {
      dg[w] = 0xffffffffu;
      if (!CW && w >= nwin) continue;
      const uint32_t d = signed_digit(v, w, c, carry, neg);
      if (d) {
        dg[w] = (d - 1) | (neg << 31);
        atomicAdd(&hist[(d - 1) >> shift], 1u);
      }
    }
  }
  __syncthreads();
  wave0_scan<PART_MAX>(hist, lstart);
  if (t < npart) {
    const uint32_t h = hist[t];
    gbase[t] = h ? poff[m * npart + t] + atomicAdd(&pcursor[m * npart + t], h) : 0u;
  }
  __syncthreads();
  const uint32_t total = lstart[PART_MAX - 1] + hist[PART_MAX - 1];
  __syncthreads();
  if (t < PART_MAX) hist[t] = 0;
  __syncthreads();
#pragma unroll
  for (uint32_t w = 0; w < (CW ? NW : PSC_MAX_WIN); w++) {
    if (dg[w] == 0xffffffffu) continue;
    const uint32_t bk = dg[w] & 0x7fffffffu;
    const uint32_t pt = bk >> shift;
    // entry: point index (26 bits) | window << 26 | sign << 31, and the bucket inside the MSM
    stage[lstart[pt] + atomicAdd(&hist[pt], 1u)] = make_uint2(i | (w << 26) | (dg[w] & 0x80000000u), bk);
  }
  __syncthreads();
  // 5 bytes per entry leave the chunk: the payload and, in a byte array of its own, the bucket inside the partition (the
  // bucket-count pass then reads one byte per entry, the placement pass five, instead of eight each)
  for (uint32_t j = t; j < total; j += PSC_THREADS) {
    const uint2 e = stage[j];
    const uint32_t pt = e.y >> shift;
    const uint32_t dst = gbase[pt] + (j - lstart[pt]);
    part_pay[dst] = e.x;
    part_low[dst] = (LowT)(e.y & ((1u << shift) - 1u));
  }
}

// ---- one LDS sort for the bucket passes and the refinement passes ------------------------------------------------
// Both levels below the partition pass count the entries of a partition per BIN and then place them, tile by tile, as
// per-bin runs.  A policy says what differs:
//   Low          the incoming low part of an entry (what the pass before left of its bucket);
//   CELLS, rlog  the LDS histogram: a bin owns 1 << rlog adjacent cells, an entry counts in cell (bin << rlog) | rep;
//   bins_log     the pass's 1 << bins_log bins per partition: bin b of partition pid is entry (pid << bins_log) + b of
//                the arrays the runs are reserved against;
//   bin(low), emit(dst, payload, low)   an entry's bin, and what leaves the tile.
// Bucket passes: partition pid = msm * npart + p owns the flat buckets [pid << PB, (pid + 1) << PB) (PB: bits of the bucket
// inside a partition, 7 or 8); the bin is the bucket, one cell each, and the payload alone goes into the bucket's list.
template <uint32_t PB>
struct BucketBins {
  using Low = uint8_t;
  static constexpr uint32_t CELLS = 1u << PB, bins_log = PB, rlog = 0, rep = 0;
  uint32_t* sorted;
  __device__ __forceinline__ uint32_t bin(uint32_t low) const { return low; }
  __device__ __forceinline__ void emit(uint32_t dst, uint32_t pay, uint32_t) const { sorted[dst] = pay; }
};
// Wide windows (c > 17, 2^(c-1) buckets per MSM): the first pass still cuts an MSM into 128 partitions -- now of
// 2^(c-8) buckets -- and a REFINEMENT pass of the same shape as the bucket passes splits every such partition into
// its 2^(c-15) final partitions of 128 buckets, which the bucket passes then finish.  The few bins of a partition are
// spread over 128 histogram cells (bin, thread mod R) so that the LDS atomics of a wave do not pile up on 2..32
// addresses; cells of one bin are adjacent, so the LDS-sorted tile is still a sequence of per-bin runs.  The payload and
// the remaining 7 bits leave the tile.
struct RefineBins {
  using Low = uint16_t;
  static constexpr uint32_t CELLS = PART_BUCKETS;
  uint32_t bins_log, rlog, rep;
  uint32_t* pay2;
  uint8_t* low2;
  __device__ __forceinline__ RefineBins(uint32_t bins_log_, uint32_t* pay2_ = nullptr, uint8_t* low2_ = nullptr)
      : bins_log(bins_log_), rlog(PART_BITS - bins_log_), rep(threadIdx.x & ((1u << rlog) - 1u)), pay2(pay2_), low2(low2_) {}
  __device__ __forceinline__ uint32_t bin(uint32_t low) const { return low >> PART_BITS; }
  __device__ __forceinline__ void emit(uint32_t dst, uint32_t pay, uint32_t low) const {
    pay2[dst] = pay;
    low2[dst] = (uint8_t)(low & (PART_BUCKETS - 1));
  }
};
template <class P>
static __device__ __forceinline__ uint32_t bin_count(const P& p, const uint32_t* hist, uint32_t bin) {
  uint32_t sum = 0;
  for (uint32_t r = 0; r < (1u << p.rlog); r++) sum += hist[(bin << p.rlog) + r];
  return sum;
}

// LDS histogram of the partition's entries (gridDim.y workgroups share it), one device atomic per non-empty bin
template <class P>
static __device__ __forceinline__ void part_count(const P& p, const typename P::Low* __restrict__ low, const uint32_t* __restrict__ poff,
                                                  uint32_t* __restrict__ bin_sizes) {
  __shared__ uint32_t hist[P::CELLS];
  const uint32_t pid = blockIdx.x, t = threadIdx.x;
  const uint32_t lo = poff[pid], hi = poff[pid + 1];
  if (lo + blockIdx.y * PART_THREADS >= hi) return;  // block-uniform
  if (t < P::CELLS) hist[t] = 0;
  __syncthreads();
  for (uint32_t e = lo + blockIdx.y * PART_THREADS + t; e < hi; e += gridDim.y * PART_THREADS)
    atomicAdd(&hist[(p.bin(low[e]) << p.rlog) | p.rep], 1u);
  __syncthreads();
  if (t < (1u << p.bins_log)) {
    const uint32_t h = bin_count(p, hist, t);
    if (h) atomicAdd(&bin_sizes[(pid << p.bins_log) + t], h);
  }
}

// A tile's entries are sorted by bin in LDS, then copied out run by run (bucket passes: ~32 entries = one 128-byte line
// per bucket and tile): LDS histogram, scan, one device atomic per non-empty bin to reserve the tile's run behind
// bin_start + what bin_cursor holds, placement in LDS, linear copy.  gridDim.y workgroups share a partition tile by tile.
template <class P>
static __device__ __forceinline__ void part_tile_place(const P& p, const uint32_t* __restrict__ pay, const typename P::Low* __restrict__ low,
                                                       const uint32_t* __restrict__ poff, const uint32_t* __restrict__ bin_start,
                                                       uint32_t* __restrict__ bin_cursor) {
  constexpr uint32_t NC = P::CELLS;
  __shared__ uint32_t hist[NC], lstart[NC], base[NC];
  __shared__ uint32_t spay[PART_TILE];
  __shared__ typename P::Low slow[PART_TILE];
  const uint32_t pid = blockIdx.x, t = threadIdx.x;
  const uint32_t lo = poff[pid], hi = poff[pid + 1];
  const uint32_t ntiles = (hi - lo + PART_TILE - 1) / PART_TILE;
  for (uint32_t tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {  // block-uniform trip count
    const uint32_t tlo = lo + tile * PART_TILE, thi = min(hi, tlo + PART_TILE);
    if (t < NC) hist[t] = 0;
    __syncthreads();
    uint2 ent[PART_PER_LANE];
#pragma unroll
    for (uint32_t k = 0; k < PART_PER_LANE; k++) {
      const uint32_t e = tlo + k * PART_THREADS + t;
      if (e < thi) {
        ent[k] = make_uint2(pay[e], low[e]);
        atomicAdd(&hist[(p.bin(ent[k].y) << p.rlog) | p.rep], 1u);
      }
    }
    __syncthreads();
    wave0_scan<NC>(hist, lstart);
    if (t < (1u << p.bins_log)) {  // the tile's run inside bin (pid, t)
      const uint32_t h = bin_count(p, hist, t), g = (pid << p.bins_log) + t;
      base[t] = h ? bin_start[g] + atomicAdd(&bin_cursor[g], h) : 0u;
    }
    __syncthreads();
    if (t < NC) hist[t] = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < PART_PER_LANE; k++) {
      const uint32_t e = tlo + k * PART_THREADS + t;
      if (e < thi) {
        const uint32_t cell = (p.bin(ent[k].y) << p.rlog) | p.rep;
        const uint32_t lp = lstart[cell] + atomicAdd(&hist[cell], 1u);
        spay[lp] = ent[k].x;
        slow[lp] = (typename P::Low)ent[k].y;
      }
    }
    __syncthreads();
    for (uint32_t j = t; j < thi - tlo; j += PART_THREADS) {
      const uint32_t l = slow[j], b = p.bin(l);
      p.emit(base[b] + (j - lstart[b << p.rlog]), spay[j], l);
    }
    __syncthreads();
  }
}

template <uint32_t PB>
__global__ __launch_bounds__(PART_THREADS) void msm_bucket_count_kernel(const uint8_t* __restrict__ part_low, const uint32_t* __restrict__ poff,
                                                                        uint32_t* __restrict__ counts) {
  CQ_CRITICAL_WAVES();
  part_count(BucketBins<PB>{nullptr}, part_low, poff, counts);
}
template <uint32_t PB>
__global__ __launch_bounds__(PART_THREADS) void msm_bucket_place_kernel(const uint32_t* __restrict__ part_pay, const uint8_t* __restrict__ part_low,
                                                                        const uint32_t* __restrict__ poff,
                                                                        const uint32_t* __restrict__ off0, uint32_t* __restrict__ cursor,
                                                                        uint32_t* __restrict__ sorted) {
  CQ_CRITICAL_WAVES();
  part_tile_place(BucketBins<PB>{sorted}, part_pay, part_low, poff, off0, cursor);
}
__global__ __launch_bounds__(PART_THREADS) void msm_refine_count_kernel(const uint16_t* __restrict__ low1, const uint32_t* __restrict__ poff1,
                                                                        uint32_t bins_log, uint32_t* __restrict__ psize2) {
  part_count(RefineBins(bins_log), low1, poff1, psize2);
}
__global__ __launch_bounds__(PART_THREADS) void msm_refine_place_kernel(const uint32_t* __restrict__ pay1, const uint16_t* __restrict__ low1,
                                                                        const uint32_t* __restrict__ poff1, uint32_t bins_log,
                                                                        const uint32_t* __restrict__ poff2, uint32_t* __restrict__ cursor2,
                                                                        uint32_t* __restrict__ pay2, uint8_t* __restrict__ low2) {
  part_tile_place(RefineBins(bins_log, pay2, low2), pay1, low1, poff1, poff2, cursor2);
}

// an MSM that accumulates from another one's lists (same scalar vector) takes a copy of its bucket counts
__global__ __launch_bounds__(256) void msm_alias_counts_kernel(uint32_t* __restrict__ counts, const uint64_t* __restrict__ list_src, uint32_t B) {
  CQ_CRITICAL_WAVES();
  const uint32_t m = blockIdx.y, src = (uint32_t)list_src[m];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (src != m && i < B) counts[(size_t)m * B + i] = counts[(size_t)src * B + i];
}

// ---- index front (bucket-sum launches): the "scalars" are bucket numbers already ---------------------------------------
// index[i] = b < count puts row i into bucket b of its MSM, any other value nowhere: one entry per row at most, window 0,
// no sign -- the payload is the row number.  Nothing has to be reduced, cut into digits or routed through partitions: one
// kernel counts, one places behind the plan's list starts.  Both work on tiles of INDEX_TILE rows per workgroup and keep the
// tile's buckets in a small LDS hash table (open addressing, INDEX_SLOTS = 2 x INDEX_TILE slots: a tile names at most
// INDEX_TILE buckets, so a probe always ends at its own key or at a free slot), whatever `count` is.  What reaches L2 is one
// device atomic per (tile, bucket named in it): a witness whose padded rows all look up one table row costs that bucket one
// atomic per tile -- 128 per list at k = 18 -- where an atomic per wave would be 4 096 of ~15 ns each.  The LDS atomics are
// thinned the same way: lanes of a wave that share a bucket send one.
constexpr uint32_t INDEX_THREADS = 256, INDEX_PER_LANE = 8, INDEX_TILE = INDEX_THREADS * INDEX_PER_LANE;
constexpr uint32_t INDEX_SLOTS = 2 * INDEX_TILE, INDEX_NONE = 0xffffffffu;
constexpr uint32_t INDEX_RANK_BITS = 12;  // a placed entry: slot << INDEX_RANK_BITS | rank inside the tile's run
static_assert(INDEX_TILE <= (1u << INDEX_RANK_BITS) && INDEX_SLOTS <= (1u << (31 - INDEX_RANK_BITS)), "slot and rank share a word");

// the slot of bucket b in the tile's table, claimed on first sight
static __device__ __forceinline__ uint32_t index_slot(uint32_t* keys, uint32_t b) {
  uint32_t s = (b * 0x9e3779b1u) >> 20 & (INDEX_SLOTS - 1);
  for (uint32_t probe = 0; probe < INDEX_SLOTS; probe++) {  // (ends long before: at most INDEX_TILE slots are ever taken)
    const uint32_t prev = atomicCAS(&keys[s], INDEX_NONE, b);
    if (prev == INDEX_NONE || prev == b) break;
    s = (s + 1) & (INDEX_SLOTS - 1);
  }
  return s;
}

// counts[m * B + b] += the rows of the tile on bucket b.  A lane folds the equal neighbours among its INDEX_PER_LANE rows
// (strided, so loads stay coalesced) into a running (bucket, count) pair as cq_round1_kernel does; the pair it ends with is
// summed across the lanes that share it before it goes to LDS.  totals[m]: the list's entries; the workgroup that finishes
// last settles the launch's sub-list length from them exactly as msm_part_scan_kernel does for the generic front.
__global__ __launch_bounds__(INDEX_THREADS) void msm_index_count_kernel(const uint32_t* const* __restrict__ index, const uint64_t* __restrict__ lens,
                                                                        const uint64_t* __restrict__ list_src, uint32_t batch, uint32_t B,
                                                                        uint32_t count, uint32_t* __restrict__ counts, uint32_t* totals /* [batch] */,
                                                                        uint32_t* ticket, uint32_t s1_host, uint32_t* __restrict__ s1_out) {
  CQ_CRITICAL_WAVES();
  __shared__ uint32_t keys[INDEX_SLOTS], cnt[INDEX_SLOTS];
  __shared__ uint32_t tile_total;
  const uint32_t m = blockIdx.y, t = threadIdx.x, lane = t & 63;
  const uint32_t len = (uint32_t)lens[m];  // 0 for an MSM that reads another one's lists
  const uint32_t base = blockIdx.x * INDEX_TILE;
  if (base < len) {  // block-uniform
    for (uint32_t s = t; s < INDEX_SLOTS; s += INDEX_THREADS) {
      keys[s] = INDEX_NONE;
      cnt[s] = 0;
    }
    if (t == 0) tile_total = 0;
    __syncthreads();
    const uint32_t* __restrict__ idx = index[m];
    uint32_t bk[INDEX_PER_LANE];
#pragma unroll
    for (uint32_t k = 0; k < INDEX_PER_LANE; k++) {
      const uint32_t i = base + k * INDEX_THREADS + t;
      bk[k] = i < len ? idx[i] : INDEX_NONE;
    }
    uint32_t held = INDEX_NONE, held_cnt = 0;
#pragma unroll
    for (uint32_t k = 0; k < INDEX_PER_LANE; k++) {
      if (bk[k] >= count) continue;
      if (bk[k] == held) {
        held_cnt++;
      } else {
        if (held_cnt) atomicAdd(&cnt[index_slot(keys, held)], held_cnt);
        held = bk[k];
        held_cnt = 1;
      }
    }
    bool pending = held_cnt != 0;
#pragma unroll 1
    for (int round = 0; round < 2 && __ballot(pending); round++) {
      const int leader = __ffsll((long long)__ballot(pending)) - 1;
      const uint32_t lb = __shfl(held, leader, 64);
      const bool mine = pending && held == lb;
      uint32_t c = mine ? held_cnt : 0u;
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
      if ((int)lane == leader) atomicAdd(&cnt[index_slot(keys, lb)], c);
      if (mine) pending = false;
    }
    if (pending) atomicAdd(&cnt[index_slot(keys, held)], held_cnt);
    __syncthreads();
    uint32_t sum = 0;
    for (uint32_t s = t; s < INDEX_SLOTS; s += INDEX_THREADS) {
      const uint32_t h = cnt[s];
      if (h) atomicAdd(&counts[(size_t)m * B + keys[s]], h);
      sum += h;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == 0 && sum) atomicAdd(&tile_total, sum);
    __syncthreads();
    if (t == 0 && tile_total) atomicAdd(&totals[m], tile_total);
  }
  if (t) return;
  __threadfence();
  if (atomicAdd(ticket, 1u) != gridDim.x * gridDim.y - 1) return;
  __threadfence();
  uint64_t entries = 0;
  for (uint32_t q = 0; q < batch; q++) entries += atomicAdd(&totals[(uint32_t)list_src[q]], 0u);
  const uint32_t s1 = msm_small_launch_s1(entries);  // (the host's value stands for a launch that is not small)
  *s1_out = entries < (uint64_t)MSM_S1 * MSM_SMALL_LANES && s1 < s1_host ? s1 : s1_host;
}

// sorted[off0[m * B + b] + rank] = i for every row i of the tile on bucket b.  The rank inside the tile comes from LDS --
// lanes of a wave that share the bucket of the first (then the second) pending lane are ranked from one ballot and send one
// atomic, as in msm_digits_kernel; the rest send their own -- and the tile's run inside the bucket's list is reserved with
// one device atomic on `cursor` per bucket the tile names.  Lanes ranked together write consecutive words.
__global__ __launch_bounds__(INDEX_THREADS) void msm_index_place_kernel(const uint32_t* const* __restrict__ index, const uint64_t* __restrict__ lens,
                                                                        uint32_t B, uint32_t count, const uint32_t* __restrict__ off0,
                                                                        uint32_t* __restrict__ cursor, uint32_t* __restrict__ sorted) {
  CQ_CRITICAL_WAVES();
  __shared__ uint32_t keys[INDEX_SLOTS], run[INDEX_SLOTS];  // run: the tile's entries on the slot's bucket, then where they go
  const uint32_t m = blockIdx.y, t = threadIdx.x, lane = t & 63;
  const uint32_t len = (uint32_t)lens[m];
  const uint32_t base = blockIdx.x * INDEX_TILE;
  if (base >= len) return;  // block-uniform
  for (uint32_t s = t; s < INDEX_SLOTS; s += INDEX_THREADS) {
    keys[s] = INDEX_NONE;
    run[s] = 0;
  }
  __syncthreads();
  const uint32_t* __restrict__ idx = index[m];
  uint32_t bk[INDEX_PER_LANE], where[INDEX_PER_LANE];
#pragma unroll
  for (uint32_t k = 0; k < INDEX_PER_LANE; k++) {
    const uint32_t i = base + k * INDEX_THREADS + t;
    bk[k] = i < len ? idx[i] : INDEX_NONE;
  }
#pragma unroll
  for (uint32_t k = 0; k < INDEX_PER_LANE; k++) {
    const bool act = bk[k] < count;
    bool pending = act, issue = act;
    uint32_t add = 1, lead = 64, below = 0;
#pragma unroll
    for (int round = 0; round < 2; round++) {
      const unsigned long long pend = __ballot(pending);
      if (pend) {  // wave-uniform
        const int leader = __ffsll((long long)pend) - 1;
        const uint32_t lb = __shfl(bk[k], leader, 64);
        const bool mine = pending && bk[k] == lb;
        const unsigned long long grp = __ballot(mine);
        if (mine) {
          lead = (uint32_t)leader;
          below = __popcll(grp & ((1ull << lane) - 1ull));
          add = __popcll(grp);
          issue = (int)lane == leader;
          pending = false;
        }
      }
    }
    uint32_t slot = 0, first = 0;
    if (issue) {
      slot = index_slot(keys, bk[k]);
      first = atomicAdd(&run[slot], add);
    }
    const uint32_t lslot = __shfl(slot, lead & 63, 64), lfirst = __shfl(first, lead & 63, 64);  // every lane takes part
    if (lead < 64) {
      slot = lslot;
      first = lfirst + below;
    }
    where[k] = act ? (slot << INDEX_RANK_BITS) | first : INDEX_NONE;
  }
  __syncthreads();
  for (uint32_t s = t; s < INDEX_SLOTS; s += INDEX_THREADS) {
    const uint32_t h = run[s];
    if (h) {
      const size_t g = (size_t)m * B + keys[s];
      run[s] = off0[g] + atomicAdd(&cursor[g], h);
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < INDEX_PER_LANE; k++)
    if (where[k] != INDEX_NONE)
      sorted[run[where[k] >> INDEX_RANK_BITS] + (where[k] & ((1u << INDEX_RANK_BITS) - 1u))] = base + k * INDEX_THREADS + t;
}

// ---- 3. scatter (counting sort) ----------------------------------------------------------------
// Recomputes the digits (cheaper than storing them) and drops every entry at list start + rank.
__global__ __launch_bounds__(256) void msm_scatter_kernel(const Fr* const* __restrict__ scalars, const uint64_t* __restrict__ lens,
                                                          uint32_t nmax, uint32_t c, uint32_t nwin, uint32_t pre,
                                                          const uint32_t* __restrict__ ranks, const uint32_t* __restrict__ off0,
                                                          uint32_t* __restrict__ sorted) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t m = blockIdx.y;
  if (i >= (uint32_t)lens[m]) return;
  const U256 v = scalars[m][i].to_canonical();
  const uint32_t M = 1u << (c - 1);
  uint32_t carry = 0, neg;
  for (uint32_t w = 0; w < nwin; w++) {
    const uint32_t d = signed_digit(v, w, c, carry, neg);
    if (!d) continue;
    const size_t mw = (size_t)m * nwin + w;
    const uint32_t g = (uint32_t)((pre ? (size_t)m : mw) * M) + (d - 1);
    // entry: point index (26 bits) | window << 26 (precomputed-table mode) | sign << 31
    sorted[off0[g] + ranks[mw * nmax + i]] = i | (pre ? (w << 26) : 0u) | (neg << 31);
  }
}

// the partition pass of a table-mode launch: histogram, scan (which also settles the launch's s1), scatter
struct PartPass1 {
  hipStream_t s;
  dim3 hgrid, sgrid;
  const Fr* const* scalars;
  const uint64_t *lens, *list_src;
  uint32_t c, W, npart, per_lane, batch, s1, P;
  uint32_t *psize /* [P] sizes, [P] cursors */, *poff, *s1_dev, *part_pay;
  void* part_low;
};
template <uint32_t CW, uint32_t NW, typename LowT>
static void launch_part_pass1(const PartPass1& a) {
  msm_part_hist_kernel<CW, NW><<<a.hgrid, DIGITS_LDS_THREADS, 0, a.s>>>(a.scalars, a.lens, a.c, a.W, a.npart, a.per_lane, a.psize);
  msm_part_scan_kernel<<<1, 1024, 0, a.s>>>(a.psize, a.P, a.poff, a.list_src, a.batch, a.npart, a.s1, a.s1_dev);
  msm_part_scatter_kernel<CW, NW, LowT><<<a.sgrid, PSC_THREADS, 0, a.s>>>(a.scalars, a.lens, a.c, a.W, a.npart, a.poff, a.psize + a.P, a.part_pay,
                                                                          (LowT*)a.part_low);
}

void msm_enqueue_tables(hipStream_t s, const MsmLayout& L, const MsmBuffers& b, const MsmTableRows& rows) {
  // counts and the sort's cursors are adjacent (and 256-byte aligned): cleared by the same kernel
  const size_t quads = b.zero_quads;
  const uint32_t blocks = (uint32_t)std::min<size_t>((quads + 255) / 256, 1024);
  msm_set_ptrs_kernel<<<std::max(blocks, 1u), 256, 0, s>>>(rows.lists, rows.bases, rows.strides, rows.lens, rows.src, b.ptrs, L.batch, (uint4*)b.counts, quads);
}

void msm_front_plain(hipStream_t s, const MsmLayout& L, const MsmBuffers& b, uint32_t s1) {
  const uint32_t n = L.n, c = L.c, W = L.W, batch = L.batch;
  msm_digits_kernel<<<dim3((n + 255) / 256, batch), 256, 0, s>>>(b.scalars(), b.lens, n, c, W, L.pre ? 1u : 0u, b.ranks, b.counts);
  msm_plan(s, L, b, s1, nullptr);
  msm_scatter_kernel<<<dim3((n + 255) / 256, batch), 256, 0, s>>>(b.scalars(), b.lens, n, c, W, L.pre ? 1u : 0u, b.ranks, b.off, b.sorted);
}

// count -> plan -> place over the rows of every list source (see "index front"); the region of the partition sizes,
// cleared with the counts, holds the lists' totals and the count kernel's ticket
void msm_front_index(hipStream_t s, const MsmLayout& L, const MsmBuffers& b, uint32_t s1, bool any_alias, uint32_t count) {
  const uint32_t batch = L.batch;
  const dim3 grid((L.n + INDEX_TILE - 1) / INDEX_TILE, batch);
  msm_index_count_kernel<<<grid, INDEX_THREADS, 0, s>>>(b.index(), b.lens, b.src, batch, L.B, count, b.counts, b.totals, b.index_ticket, s1, b.s1_dev);
  if (any_alias) msm_alias_counts_kernel<<<dim3((L.B + 255) / 256, batch), 256, 0, s>>>(b.counts, b.src, L.B);
  msm_plan(s, L, b, s1, b.s1_dev);
  msm_index_place_kernel<<<grid, INDEX_THREADS, 0, s>>>(b.index(), b.lens, L.B, count, b.off, b.cursor, b.sorted);
}

void msm_front_partition(hipStream_t s, const MsmLayout& L, const MsmBuffers& b, uint32_t s1, bool any_alias) {
  const uint32_t n = L.n, c = L.c, W = L.W, batch = L.batch;
  const uint32_t P = batch * L.npart;
  // scalars per lane of the partition histogram: few in a small launch (more workgroups in flight: the kernel is
  // latency-bound there), DIGITS_LDS_PER_LANE in a large one (fewer device atomics: 128 per workgroup)
  const uint32_t per_lane = (uint64_t)n * batch <= (1u << 21) ? 2u : DIGITS_LDS_PER_LANE;
  const uint32_t hist_chunk = DIGITS_LDS_THREADS * per_lane;
  const dim3 hgrid((n + hist_chunk - 1) / hist_chunk, batch), sgrid((n + PSC_THREADS - 1) / PSC_THREADS, batch);
  // window width and count as compile-time constants for the table widths in use (see msm_part_hist_kernel)
  const PartPass1 pp{s, hgrid, sgrid, b.scalars(), b.lens, b.src, c, W, L.npart, per_lane, batch, s1, P, b.psize, b.poff, b.s1_dev, b.part_pay, b.part_low};
  if (c == 15 && W == 17) launch_part_pass1<15, 17, uint8_t>(pp);
  else if (c == 16 && W == 16) launch_part_pass1<16, 16, uint8_t>(pp);
  else if (c == 17 && W == 15) launch_part_pass1<17, 15, uint8_t>(pp);
  else if (c == 18 && W == 15) launch_part_pass1<18, 15, uint16_t>(pp);
  else if (c == 19 && W == 14) launch_part_pass1<19, 14, uint16_t>(pp);
  else if (c == 20 && W == 13) launch_part_pass1<20, 13, uint16_t>(pp);
  else if (L.mid) launch_part_pass1<0, 0, uint16_t>(pp);
  else launch_part_pass1<0, 0, uint8_t>(pp);
  // workgroups per partition in the bucket passes: PART_SPLIT when partitions hold many tiles, one when they hold one
  auto split_for = [&](uint32_t parts) {
    const uint64_t tiles = (uint64_t)W * n * batch / ((uint64_t)parts * PART_TILE) + 1;
    return (uint32_t)std::min<uint64_t>(PART_SPLIT, tiles);
  };
  const uint32_t* fpay = b.part_pay;
  const uint8_t* flow = (const uint8_t*)b.part_low;
  const uint32_t* fpoff = b.poff;
  uint32_t F = P;
  if (L.mid) {  // 128 partitions of 2^(c-8) buckets -> partitions of 128 buckets
    const uint16_t* low1 = (const uint16_t*)b.part_low;
    F = batch * L.nfinal;
    const uint32_t bins_log = L.shift1 - PART_BITS;
    msm_refine_count_kernel<<<dim3(P, PART_SPLIT), PART_THREADS, 0, s>>>(low1, b.poff, bins_log, b.psize2);
    msm_part_scan_kernel<<<1, 1024, 0, s>>>(b.psize2, F, b.poff2);
    msm_refine_place_kernel<<<dim3(P, PART_SPLIT), PART_THREADS, 0, s>>>(b.part_pay, low1, b.poff, bins_log, b.poff2, b.psize2 + F, b.pay2, b.low2);
    fpay = b.pay2;
    flow = b.low2;
    fpoff = b.poff2;
  }
  const uint32_t split = split_for(F);
  const bool wide = !L.mid && L.shift1 == PART_BITS_WIDE;  // 256 buckets per partition
  if (wide) msm_bucket_count_kernel<PART_BITS_WIDE><<<dim3(F, split), PART_THREADS, 0, s>>>(flow, fpoff, b.counts);
  else msm_bucket_count_kernel<PART_BITS><<<dim3(F, split), PART_THREADS, 0, s>>>(flow, fpoff, b.counts);
  if (any_alias) msm_alias_counts_kernel<<<dim3((L.B + 255) / 256, batch), 256, 0, s>>>(b.counts, b.src, L.B);
  msm_plan(s, L, b, s1, b.s1_dev);
  if (wide) msm_bucket_place_kernel<PART_BITS_WIDE><<<dim3(F, split), PART_THREADS, 0, s>>>(fpay, flow, fpoff, b.off, b.cursor, b.sorted);
  else msm_bucket_place_kernel<PART_BITS><<<dim3(F, split), PART_THREADS, 0, s>>>(fpay, flow, fpoff, b.off, b.cursor, b.sorted);
}

}  // namespace cq

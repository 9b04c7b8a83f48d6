// Workspace description of one launch of the G1 MSM engine (msm.hip): what the launch's shape fixes -- windows, bucket
// sets, combine levels, which sorting front it takes -- and where every region of its workspace starts.  Host-only and free
// of HIP, so that a plain C++ compiler builds it (tests/host/msm_layout_check.cpp); MsmBuffers (msm.hpp) turns the offsets
// into the typed pointers the kernels are handed, in one place.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace cq {

// What the arithmetic below needs of the engine, restated as constants: the byte sizes of an XYZZ point (the only point type
// the workspace holds; G1Affine arrays are the callers') and of a device pointer, and the tuning constants of msm.hpp (whose
// -D overrides are followed).  msm.hip static_asserts every one against the real thing.
namespace msm_layout_k {
constexpr size_t XYZZ_BYTES = 128, PTR_BYTES = 8;
#ifdef CQ_MSM_S1
constexpr uint32_t S1 = CQ_MSM_S1;
#else
constexpr uint32_t S1 = 24;
#endif
#ifdef CQ_MSM_SMALL_LANES
constexpr uint64_t SMALL_LANES = CQ_MSM_SMALL_LANES;
#else
constexpr uint64_t SMALL_LANES = 65536;
#endif
constexpr uint32_t S1_MIN = 4, S2 = 64, SHORT_MIN = 16, TABLE_C_MAX = 20;
constexpr uint64_t SMALL_PARTIALS = 3 * SMALL_LANES;
}  // namespace msm_layout_k

// Small launches (fewer than MSM_SMALL_LANES sub-lists of MSM_S1 entries): shorter sub-lists, down to MSM_S1_MIN, so that
// the accumulate kernel -- a chain of dependent additions per lane, ~7 us each -- has a lane per few entries instead of
// 17-24 of them on a fraction of the SIMDs (k = 14: one 16 384-term MSM was 140 us of pure latency).  A function of the
// launch's entry BOUND (batch x windows x n), so that the workspace layout and the launch agree.  (constexpr: the kernels
// that settle a launch's own value call it too.)
constexpr uint32_t msm_small_launch_s1(uint64_t entry_bound) {
  if (entry_bound >= (uint64_t)msm_layout_k::S1 * msm_layout_k::SMALL_LANES) return msm_layout_k::S1;
  const uint64_t s = entry_bound / msm_layout_k::SMALL_LANES;
  return (uint32_t)(s < msm_layout_k::S1_MIN ? msm_layout_k::S1_MIN : s);
}

// The partition sort's shape (msm_sort.hip), as far as the layout depends on it.
constexpr uint32_t DIGITS_LDS_MAX_M = 1u << 14;
constexpr uint32_t PART_BITS = 7, PART_BUCKETS = 1u << PART_BITS;  // buckets per partition (c <= 15 and behind a refinement pass)
constexpr uint32_t PART_BITS_WIDE = 8;                             // ... 256 of them for c = 16 and c = 17
constexpr uint32_t PSC_MAX_WIN = 17;                               // windows msm_part_scatter_kernel keeps digits for
// `shift`: bucket -> partition of the first pass (PART_BITS up to c = 15; c - 8, i.e. always 128 partitions, beyond)
constexpr uint32_t part_shift_of(uint32_t c) { return c > 17 ? c - 8 : c > 15 ? PART_BITS_WIDE : PART_BITS; }

// Workspace carve-up for `batch` MSMs of n terms each with c-bit signed windows.
struct MsmLayout {
  // M: buckets per bucket SET (the reduction's rows x cols matrix), Wb: sets per MSM, B = Wb * M: buckets per MSM.
  // Table mode has one set per MSM up to c = 15 (M = 2^(c-1)) and 2^(c-15) sets of 2^14 buckets for wider windows.
  uint32_t n, c, batch, W, Wb, M, B, Bt, levels, nseq, nblk, rows, cols, npart, nfinal, shift1;
  bool pre, part_sort, mid;
  uint64_t E;  // upper bound on (point,digit) entries
  uint64_t tmax[8];
  // Regions, in this order, each on a 256-byte boundary.  counts .. ticket (up to zero_end) are cleared by the launch's first
  // kernel.  Regions with more than one user, and the sub-regions below, are spelled out at MsmBuffers.
  size_t off_ptrs, off_ranks, off_poff, off_poff2, off_counts, off_cursor, off_psize, off_psize2, off_ticket, zero_end, off_buckets, off_blocksums,
      off_off, off_tk, off_sorted, off_part[2], off_pairs, total;
  inline MsmLayout(uint32_t n_, uint32_t c_, uint32_t batch_, bool pre_ = false);

  // ---- sub-regions: where a region's several users sit inside it ----
  // off_ptrs: five rows of `batch` 8-byte entries (msm_set_ptrs_kernel): lists, bases, strides, lens, src
  size_t off_ptr_row(uint32_t row) const { return off_ptrs + (size_t)row * batch * msm_layout_k::PTR_BYTES; }
  // off_ranks, table mode.  Two passes: pay (4 E bytes) | low, a byte per entry.  With the refinement pass: pay | pay2 | low1
  // (u16) | low2 (u8), the 32-bit arrays first so that both stay 4-byte aligned whatever the parity of E
  size_t off_part_pay() const { return off_ranks; }
  size_t off_pay2() const { return off_ranks + (size_t)E * 4; }  // (mid only)
  size_t off_part_low() const { return off_ranks + (size_t)E * (mid ? 8 : 4); }
  size_t off_low2() const { return off_part_low() + (size_t)E * 2; }  // (mid only)
  // off_blocksums: behind the nseq x nblk tile totals, the sub-list length the launch settles on
  size_t off_s1_dev() const { return off_blocksums + (size_t)nseq * nblk * sizeof(uint32_t); }
  // off_psize, index front: the lists' totals, then the count kernel's ticket
  size_t off_index_ticket() const { return off_psize + (size_t)batch * sizeof(uint32_t); }
};

MsmLayout::MsmLayout(uint32_t n_, uint32_t c_, uint32_t batch_, bool pre_) : n(n_), c(c_), batch(batch_), pre(pre_) {
  using namespace msm_layout_k;
  constexpr uint32_t MSM_S1_MIN = S1_MIN, MSM_S2 = S2, MSM_SHORT_MIN = SHORT_MIN, MSM_TABLE_C_MAX = TABLE_C_MAX;
  constexpr uint64_t MSM_SMALL_PARTIALS = SMALL_PARTIALS;
  struct XYZZ { char b[XYZZ_BYTES]; };
  W = (255 + c - 1) / c;  // signed digits need W*c >= 255 for 254-bit scalars
  // bucket sets per MSM: one per window in plain mode; with per-window tables every window feeds the same 2^(c-1)
  // buckets, kept as sets of at most 2^14 for the reduction
  M = pre && c > 15 ? 1u << 14 : 1u << (c - 1);
  Wb = pre ? (1u << (c - 1)) / M : W;
  B = Wb * M;
  Bt = batch * B;
  levels = 1;
  {
    uint64_t cap = msm_small_launch_s1((uint64_t)batch * W * n);
    const uint64_t maxlist = pre ? (uint64_t)n * W : n;  // longest possible bucket list
    while (cap < maxlist) { cap *= MSM_S2; levels++; }
    // a launch that turns out to hold few entries cuts shorter sub-lists (msm_part_scan_kernel): a list is then at most
    // MSM_SMALL_PARTIALS partial sums long whatever its length
    uint32_t lv2 = 1;
    for (uint64_t t = std::min<uint64_t>((maxlist + MSM_S1_MIN - 1) / MSM_S1_MIN, MSM_SMALL_PARTIALS); t > 1; t = (t + MSM_S2 - 1) / MSM_S2) lv2++;
    levels = std::max(levels, lv2);
  }
  nseq = levels + 1;
  nblk = (Bt + 2047) / 2048;
  cols = M < 128 ? M : 128;  // bucket matrix of the reduction (msm_rowcol_kernel)
  rows = M / cols;
  auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
  E = (uint64_t)batch * W * n;
  size_t o = 0;
  off_ptrs = o;    o = up(o + (size_t)5 * batch * sizeof(void*));
  // table mode: (payload, bucket) pairs of the partition pass; plain mode: one rank per entry
  part_sort = pre && B <= (DIGITS_LDS_MAX_M << (MSM_TABLE_C_MAX - 15)) && B >= PART_BUCKETS && W <= PSC_MAX_WIN;
  mid = part_sort && c > 17;               // c = 16, 17: two passes with 256 buckets per partition
  shift1 = part_shift_of(c);
  npart = part_sort ? B >> shift1 : 0;     // partitions of the first pass (<= PART_MAX)
  nfinal = part_sort ? (mid ? B >> PART_BITS : npart) : 0;  // partitions the bucket passes work on
  // table mode: E payloads and E partition-local buckets (a byte each; with a refinement pass 16 bits, and a second pair
  // of arrays for its output)
  off_ranks = o;   o = up(o + (size_t)E * (part_sort ? (mid ? 11 : 5) : sizeof(uint32_t)));
  off_poff = o;    o = up(o + ((size_t)batch * npart + 1) * sizeof(uint32_t));
  off_poff2 = o;   o = up(o + (mid ? (size_t)batch * nfinal + 1 : 0) * sizeof(uint32_t));
  off_counts = o;  o = up(o + (size_t)Bt * sizeof(uint32_t));
  off_cursor = o;  o = up(o + (part_sort ? (size_t)Bt : 0) * sizeof(uint32_t));        // per-bucket fill cursors
  off_psize = o;   o = up(o + (size_t)2 * batch * npart * sizeof(uint32_t));          // partition sizes, cursors
  off_psize2 = o;  o = up(o + (mid ? (size_t)2 * batch * nfinal : 0) * sizeof(uint32_t));
  off_ticket = o;  o = up(o + sizeof(uint32_t));  // msm_scan_reduce_kernel's last-block ticket
  zero_end = o;    // counts .. ticket are cleared by the launch's first kernel; the buckets are not (msm_rowcol_kernel)
  off_buckets = o; o = up(o + (size_t)Bt * sizeof(XYZZ));
  off_blocksums = o; o = up(o + ((size_t)nseq * nblk + 1) * sizeof(uint32_t));  // + the launch's own s1 (msm_part_scan_kernel)
  off_off = o;     o = up(o + (size_t)nseq * (Bt + 1) * sizeof(uint32_t));
  off_tk = o;      o = up(o + (size_t)levels * Bt * sizeof(uint32_t));
  off_sorted = o;  o = up(o + (size_t)E * sizeof(uint32_t));
  // partial sums: level 1 has at most ceil(E/S1) + Bt sub-lists; level k >= 2 only reserves slots for lists of more
  // than MSM_SHORT_MIN items, so at most items/S2 + items/SHORT_MIN + 1 sub-lists
  for (uint32_t k = 0; k < 8; k++) tmax[k] = 0;
  const uint32_t s1_min = msm_small_launch_s1(E);  // MSM_S1 unless the launch is small (msm.hpp)
  tmax[0] = std::max<uint64_t>((E + s1_min - 1) / s1_min, std::min<uint64_t>((E + MSM_S1_MIN - 1) / MSM_S1_MIN, MSM_SMALL_PARTIALS)) + Bt;
  for (uint32_t k = 1; k < levels; k++) tmax[k] = tmax[k - 1] / MSM_S2 + tmax[k - 1] / MSM_SHORT_MIN + 1;
  off_part[0] = o;
  o = up(o + (size_t)tmax[0] * sizeof(XYZZ));
  off_part[1] = o;
  o = up(o + (size_t)(levels > 1 ? tmax[1] : 0) * sizeof(XYZZ));
  off_pairs = o;   o = up(o + (size_t)batch * Wb * (rows + cols) * sizeof(XYZZ));
  total = o;
}

}  // namespace cq

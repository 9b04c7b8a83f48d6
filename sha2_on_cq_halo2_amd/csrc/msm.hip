// Pippenger multi-scalar multiplication on BN254 G1 for gfx950 -- replaces `best_multiexp`
// (halo2_proofs/src/arithmetic.rs:132-159, serial core :13-101) and therefore
// `ParamsKZG::commit` / `commit_lagrange` (poly/kzg/commitment.rs:496-504,539-543).
//
// The reference chunks the input per CPU thread and runs unsigned c=ceil(ln n)-bit windows with
// `None/Affine/Projective` buckets.  None of that shape survives here; only the result (a group
// element, canonical once normalised) has to match.  A launch handles a BATCH of independent
// MSMs of equal length (e.g. all advice columns of a phase, plonk/prover.rs:356-360); every
// (msm, window, bucket) triple is one entry of a flat bucket array, so the batch only adds
// parallelism.  GPU pipeline, all on one stream (steps 1-3: msm_sort.hip, 4-5:
// msm_accumulate.hip, 6 and the driver that enqueues them: this file; the workspace they share: msm_layout.hpp, MsmBuffers):
//   1. digits    : scalar -> canonical (one Montgomery reduction) -> SIGNED c-bit digits (halves the bucket
//                  count).  An entry = (point, window, sign) of a non-zero digit; its bucket = |digit| - 1.
//   2. sort      : counting sort of the entries by bucket.  Table mode: two passes through LDS (partition = bucket
//                  >> 7, then bucket), every global write a run of consecutive entries -- see "Precomputed-table
//                  mode" below.  Plain mode: one device atomic per entry (issued back to back) whose return value
//                  is the entry's rank, then a scatter to list start + rank.
//   3. plan      : exclusive scans of the histogram (reduce / spine / apply): where each bucket's index list
//                  starts, and how many bounded sub-lists it is cut into per level.
//   4. accumulate: level 1 -- one lane per sub-list of <= MSM_S1 entries gathers affine points (64 B each, from
//                  the per-window tables or the caller's array) into an XYZZ accumulator (8M+2S per mixed add,
//                  no inversion) on the lazy 9x29-bit field (curve29.hpp); the next point's gather is in flight
//                  while the current addition runs.  Levels >= 2: one to four LANES per short list of partial sums
//                  (indexed by bucket), one WAVE per long one (strided lane sums + 6-step shuffle tree).  A bucket is written as soon
//                  as one lane/wave owns all of it.  Bounding the per-lane work keeps the kernel balanced for
//                  skewed digit distributions (0/1 selector columns, SHA limb columns) where a lane-per-bucket
//                  kernel would serialise on one huge bucket.  256-bit modular integer work: VALU-bound, MFMA
//                  does not apply.
//   5. reduce    : sum_b b*B_b per bucket set, shaped for depth: buckets as a rows x cols matrix, 16 lanes per
//                  row / column sum, then two weighted wave sums (the reference does this serially,
//                  arithmetic.rs:95-99).
//   6. host      : table mode returns one Jacobian point per MSM; plain mode W window sums per MSM, folded by a
//                  Horner over windows (c doublings each) on the host.
// Plain-mode MSMs of at most MSM_SHORT_MAX terms skip all of that: msm_short_kernel (msm_short.hip), one workgroup per (MSM,
// 8-bit window).  Which MSMs share a launch, and the table registry: msm_multi.hip.
// Which front a launch takes (plain digits, the partition sort with 128 or 256 buckets per partition, or that sort behind a
// refinement pass) is MsmLayout's decision, msm_layout.hpp.  Its lines, quoted for the reader of the driver (the CPU tests
// hold the quotation to the header, tests/test_msm_digits_cpu.py):
//     PSC_MAX_WIN = 17, DIGITS_LDS_MAX_M = 1u << 14, PART_BITS = 7, PART_BITS_WIDE = 8
//     part_shift_of(uint32_t c) { return c > 17 ? c - 8 : c > 15 ? PART_BITS_WIDE : PART_BITS; }
//     part_sort = pre && B <= (DIGITS_LDS_MAX_M << (MSM_TABLE_C_MAX - 15)) && B >= PART_BUCKETS && W <= PSC_MAX_WIN;
//     mid = part_sort && c > 17;
// Bucket-sum launches (msm_bucket_sums) are given bucket numbers instead of scalars: steps 1 and 2 are the index front's two kernels.
// What several kernels share exists once: the LDS sort of the bucket and refinement passes is part_count / part_tile_place
// (msm_sort.hip), named by a policy (BucketBins<PB>, RefineBins); the shuffle tree of the lane sums is xyzz29_tree_sum<WIDTH> and the
// four-lane sums are quad_load / quad_wave_sum / quad_block_sum / quad_store / quad_to_xyzz29, next to quad_add in curve29.hpp.
#include <algorithm>
#include <cstdlib>
#include "msm.hpp"
#include "curve29.hpp"
#include "ctx.hpp"

namespace cq {

uint32_t msm_window_bits(uint32_t n) {
  // Measured on MI355X (tests/perf/msm_sweep.py, uniform scalars).  15 is also the width whose top
  // window (bits 240..254) is well filled; widths that leave 1-7 bits for the top window pile
  // n/2^bits entries on a handful of buckets.  (The reference uses ceil(ln n), arithmetic.rs:16-22.)
  if (n >= (1u << 15)) return 15;
  if (n >= (1u << 13)) return 10;
  if (n >= 256) return 8;
  if (n >= 16) return 4;
  return 2;
}

// msm_layout.hpp restates what it needs of the engine as constants of its own: held to the real things here
static_assert(msm_layout_k::XYZZ_BYTES == sizeof(XYZZ) && msm_layout_k::PTR_BYTES == sizeof(void*) && sizeof(void*) == sizeof(uint64_t),
              "the layout's byte sizes");
static_assert(sizeof(G1Affine) == 64 && sizeof(uint4) == 16, "64-byte table points; the clearing kernel stores 16 bytes");
static_assert(msm_layout_k::S1 == MSM_S1 && msm_layout_k::S1_MIN == MSM_S1_MIN && msm_layout_k::S2 == MSM_S2 &&
                  msm_layout_k::SHORT_MIN == MSM_SHORT_MIN && msm_layout_k::SMALL_LANES == MSM_SMALL_LANES &&
                  msm_layout_k::SMALL_PARTIALS == MSM_SMALL_PARTIALS && msm_layout_k::TABLE_C_MAX == MSM_TABLE_C_MAX,
              "the layout's copies of the tuning constants");

// The one place where a layout offset meets the workspace pointer.
MsmBuffers::MsmBuffers(const MsmLayout& L, void* workspace) {
  char* ws = (char*)workspace;
  ptrs = (const void**)(ws + L.off_ptr_row(0));
  lists = (const void* const*)(ws + L.off_ptr_row(0));
  bases = (const G1Affine* const*)(ws + L.off_ptr_row(1));
  strides = (const uint64_t*)(ws + L.off_ptr_row(2));
  lens = (const uint64_t*)(ws + L.off_ptr_row(3));
  src = (const uint64_t*)(ws + L.off_ptr_row(4));
  counts = (uint32_t*)(ws + L.off_counts);
  cursor = (uint32_t*)(ws + L.off_cursor);
  ticket = (uint32_t*)(ws + L.off_ticket);
  zero_quads = (L.zero_end - L.off_counts) / sizeof(uint4);  // counts and the sort's cursors are adjacent (and 256-byte aligned)
  ranks = (uint32_t*)(ws + L.off_ranks);
  part_pay = (uint32_t*)(ws + L.off_part_pay());
  pay2 = L.mid ? (uint32_t*)(ws + L.off_pay2()) : nullptr;
  part_low = ws + L.off_part_low();
  low2 = L.mid ? (uint8_t*)(ws + L.off_low2()) : nullptr;
  poff = (uint32_t*)(ws + L.off_poff);
  poff2 = (uint32_t*)(ws + L.off_poff2);
  psize = (uint32_t*)(ws + L.off_psize);
  psize2 = (uint32_t*)(ws + L.off_psize2);
  totals = (uint32_t*)(ws + L.off_psize);
  index_ticket = (uint32_t*)(ws + L.off_index_ticket());
  blocksums = (uint32_t*)(ws + L.off_blocksums);
  s1_dev = (uint32_t*)(ws + L.off_s1_dev());
  off = (uint32_t*)(ws + L.off_off);
  tk = (uint32_t*)(ws + L.off_tk);
  sorted = (uint32_t*)(ws + L.off_sorted);
  buckets = (XYZZ*)(ws + L.off_buckets);
  part[0] = (XYZZ*)(ws + L.off_part[0]);
  part[1] = (XYZZ*)(ws + L.off_part[1]);
  pairs = (XYZZ*)(ws + L.off_pairs);
}

// MSMs of one launch over the SAME scalar vector (b0 and p of a CQ lookup: same coefficients, shifted bases) have
// the same entry lists: the later one is not sorted (the sort sees length 0), takes a copy of the bucket counts and
// accumulates from the earlier one's lists.  Fills the launch's tables; returns whether any MSM shares.
static bool alias_lists(const MsmLaunch& ln, const MsmLayout& L, MsmTableRows& rows) {
  uint32_t alias[MSM_MAX_BATCH];
  bool any_alias = false;
  for (uint32_t i = 0; i < MSM_MAX_BATCH; i++) {
    rows.lists.p[i] = i < L.batch ? ln.lists[i] : nullptr;
    rows.bases.p[i] = i < L.batch ? (const void*)ln.bases[i] : nullptr;
    rows.strides.s[i] = i < L.batch ? (uint64_t)ln.stride(i, L) : 0;
    rows.lens.s[i] = i < L.batch ? (uint64_t)ln.len(i, L) : 0;
    alias[i] = i;
    if (i < L.batch && L.part_sort)
      for (uint32_t j = 0; j < i; j++)
        if (alias[j] == j && ln.lists[j] == ln.lists[i] && ln.len(j, L) == ln.len(i, L) && ln.len(i, L)) {
          alias[i] = j;
          rows.lens.s[i] = 0;
          any_alias = true;
          break;
        }
    rows.src.s[i] = alias[i];
  }
  return any_alias;
}

// Sub-list length of the accumulate level, from the expected load of a bucket (entries of the launch's longest
// MSM / buckets).  Short lists keep a k = 18 launch (272 entries per bucket) parallel and balanced; with thousands
// of entries per bucket there are lanes to spare, and the partial sums per bucket must stay few: past MSM_SHORT of
// them a bucket falls to the wave-per-256 combine, which at k = 22 (4352 entries per bucket, 136 partial sums of
// 32) cost 17 ms of a 133 ms proof.  (The workspace is sized for MSM_S1, the smallest value.)
static uint32_t sublist_len(const MsmLaunch& ln, const MsmLayout& L) {
  uint64_t load = 0;
  for (uint32_t i = 0; i < L.batch; i++) load = std::max<uint64_t>(load, (uint64_t)ln.len(i, L) * L.W / (L.Wb * L.M));
  // (Longer sub-lists for the very large launches -- fewer partial sums for the combine, 2.6 ms of a k = 20 proof -- were
  // swept at k = 20 and k = 22, 32..384 entries: the accumulate kernel loses what the combine gains, within 1 %.)
  // (With several bucket sets per MSM -- wide table windows -- there are four or more times the buckets and a quarter of
  // the partial sums per bucket keeps the lanes as many: k = 22 at c = 17, 91.8 -> 90.8 ms.)
  const uint32_t partials = L.pre && L.Wb > 1 ? MSM_PARTIALS_TARGET / 4 : MSM_PARTIALS_TARGET;
  return load <= MSM_S1_BIG_LOAD ? msm_small_launch_s1(L.E) : std::max<uint32_t>(MSM_S1_BIG, (uint32_t)((load + partials - 1) / partials));
}

int msm_run(cq_ctx* ctx, const MsmLaunch& ln, const MsmLayout& L, void* workspace) {
  hipStream_t s = ctx->stream;
  const bool pre = L.pre, by_index = ln.by_index;
  const uint32_t n = L.n, batch = L.batch;
  if (by_index && (!L.part_sort || L.Wb != 1 || !ln.raw_out || ln.raw_count > L.B)) return -2;
  if (pre && (n > (1u << 26) || L.W > 32)) return -4;
  if (L.tmax[0] > 0xfffffff0ull || L.E > 0xfffffff0ull) return -3;
  if (batch == 0 || batch > MSM_MAX_BATCH) return -2;
  const MsmBuffers buf(L, workspace);
  MsmTableRows rows;
  const bool any_alias = alias_lists(ln, L, rows);
  const uint32_t s1 = sublist_len(ln, L);
  // The launch in three segments: front (pointer tables, sort, plan), the accumulate kernel, tail (combine levels, bucket
  // reduction).  Front and tail are a dozen and half a dozen small kernels whose arguments depend only on the launch's
  // shape and buffers -- the same proof after proof for a given key -- so each is captured once as a hipGraph and replayed
  // with a single hipGraphLaunch (BASELINE configs[4]: "hipGraph-captured rounds"); the accumulate kernel stays a plain
  // launch between them so that the profiling events and the side-stream hand-over (msm_tail_event) bracket it.
  auto front = [&]() -> int {
    msm_enqueue_tables(s, L, buf, rows);
    if (by_index) msm_front_index(s, L, buf, s1, any_alias, ln.raw_count);
    else if (L.part_sort) msm_front_partition(s, L, buf, s1, any_alias);
    else msm_front_plain(s, L, buf, s1);
    return 0;
  };
  auto tail = [&]() -> int {
    msm_combine_levels(s, L, buf);
    if (ln.raw_out) msm_emit_buckets(s, L, buf, ln.raw_count, ln.raw_out);  // a bucket-sum launch ends here: no weighted sum over the buckets
    else msm_reduce_sets(s, L, buf, ln.window_sums);
    return 0;
  };
  // everything the captured kernels' arguments are made of
  std::vector<uint64_t> sig{(uint64_t)(uintptr_t)workspace, (uint64_t)(uintptr_t)ln.window_sums, n, L.c, batch, (pre ? 1u : 0u) | (by_index ? 2u : 0u), s1,
                            (uint64_t)(uintptr_t)ln.raw_out, ln.raw_count};
  for (uint32_t i = 0; i < batch; i++) {
    sig.push_back((uint64_t)(uintptr_t)ln.lists[i]);
    sig.push_back((uint64_t)(uintptr_t)ln.bases[i]);
    sig.push_back((uint64_t)ln.len(i, L));
    sig.push_back((uint64_t)ln.stride(i, L));
  }
  if (ctx->run_graph(sig, 0, front) != 0) return -1;
  if (ctx->prof_on && ctx->prof_entries && ctx->prof_entries_n < cq_ctx::PROF_COUNTERS)
    (void)hipMemcpyAsync(ctx->prof_entries + ctx->prof_entries_n++, buf.off + L.Bt, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
  // Large launches release the side stream BEFORE the accumulate kernel: its lowest-priority workgroups are then placed
  // whenever the accumulate kernel has none left to place, i.e. they fill its drain (~0.3 ms of half-empty GPU at k = 22).
  // Measured (profiles/r03_msm_tail_early_ab.txt): k = 22 -0.6 .. -0.8 ms, k = 20 -0.05 .. -0.5; at k = 18 the transforms
  // that get in first delay the accumulate kernel's start by more than its shorter drain gives back (+0.25 ms on one box,
  // -0.07 on another), hence the size floor.
  constexpr size_t TAIL_EARLY_POINTS = (size_t)1 << 20;
  const bool tail_early = n >= TAIL_EARLY_POINTS;
  // (a launch on a side stream runs beside a main-stream launch and hands nothing over: the tail event and its sequence
  // number stay the main stream's, ctx.hpp.  The profiling brackets below are a pair of events of their own per launch,
  // both recorded on `s`, and the entry counter is a slot per launch: neither can pair up across streams.)
  const bool hand_over = ctx->msm_tail_event && !ctx->on_side_stream();
  if (tail_early && hand_over) {
    (void)hipEventRecord(ctx->msm_tail_event, s);
    ctx->msm_tail_seq++;
  }
  hipEvent_t pe = ctx->prof_begin(CQ_PROF_MSM_ACCUMULATE);
  msm_accumulate(s, L, buf);
  ctx->prof_end(pe);
  if (hand_over && !tail_early) {  // from here on the launch is latency-bound: side-stream work may start (ctx.hpp)
    (void)hipEventRecord(ctx->msm_tail_event, s);
    ctx->msm_tail_seq++;
  }
  if (ctx->run_graph(sig, 1, tail) != 0) return -1;
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// (The layout is the generic one of a c = 15 table launch: sized for 17 entries per scalar where this launch has one.  That
// costs address space in a grow-only buffer the round-2 launch outgrows anyway at every size in use; a shape it cannot
// hold -- msm_run's 2^32 entry bound, the 32 GiB cap of msm_multi_begin -- is refused here and the prover keeps the
// coefficient path.)
static bool bucket_sums_shape(uint32_t n, uint32_t batch) { return batch && batch <= MSM_MAX_BATCH && n && n <= (1u << 26); }
static bool bucket_sums_fit(const MsmLayout& L) { return L.E <= 0xfffffff0ull && L.tmax[0] <= 0xfffffff0ull && L.total <= ((size_t)32 << 30); }
bool msm_bucket_sums_fit(uint32_t n, uint32_t batch) { return bucket_sums_shape(n, batch) && bucket_sums_fit(MsmLayout(n, MSM_TABLE_C, batch, true)); }

int msm_bucket_sums(cq_ctx* ctx, const uint32_t* const* index, const G1Affine* const* bases29, uint32_t n, uint32_t batch, uint32_t count,
                    G1Affine* out) {
  const uint32_t c = MSM_TABLE_C;  // one bucket set of 2^(c-1) buckets per MSM, the layout of a table launch
  if (!count || count > (1u << (c - 1)) || !bucket_sums_shape(n, batch)) return -2;
  const MsmLayout L(n, c, batch, true);
  if (!bucket_sums_fit(L)) return -2;
  void* ws;
  // (beside a main-stream launch, which holds MsmWork: the side workspace, ctx.hpp)
  if (ctx->ensure_scratch(ctx->on_side_stream() ? Scratch::MsmWorkAux : Scratch::MsmWork, L.total, &ws) != 0) return -1;
  // every list has n rows, and the "tables" are one window of n points (the stride, n, is never multiplied by anything but
  // 0): both are the launch description's defaults
  const MsmLaunch ln{true, (const void* const*)index, bases29, nullptr, nullptr, nullptr, out, count};
  return msm_run(ctx, ln, L, ws);
}

// cols * V + U from the bit-plane sums of msm_weighted_kernel: V = sum_t 2^t R_t, U = sum_t 2^t C_t + C_total.
// With cols = 2^7 (every set of 2^14 buckets) the two Horner chains are one: 2^7 V + sum_t 2^t C_t is the Horner over
// R_6 .. R_0, C_6 .. C_0 -- 13 doublings and 13 additions instead of 19 and 12.
G1Jac msm_set_value(const G1Jac* planes, uint32_t cols) {
  G1Jac v = planes[6];
  for (int t = 5; t >= 0; t--) v = jac_add(jac_dbl(v), planes[t]);
  if (cols == 128) {
    for (int t = 6; t >= 0; t--) v = jac_add(jac_dbl(v), planes[7 + t]);
    return jac_add(v, planes[14]);
  }
  G1Jac u = planes[13];
  for (int t = 5; t >= 0; t--) u = jac_add(jac_dbl(u), planes[7 + t]);
  for (uint32_t l = cols; l > 1; l >>= 1) v = jac_dbl(v);
  return jac_add(jac_add(v, u), planes[14]);
}

// sum_s ( value(set s) + s * M * total(set s) ).  The value of a set is linear in its fifteen points, so the sets' points
// are added plane by plane first and folded ONCE (15 (Wb - 1) additions + 27 operations instead of 27 Wb: the host's
// share per 17-bit-window MSM goes from ~155 group operations to ~95 -- at k >= 20 the two largest host gaps of a proof).
G1Jac msm_fold_sets(const G1Jac* pairs, uint32_t Wb, uint32_t M, uint32_t cols) {
  if (Wb == 1) return msm_set_value(pairs, cols);
  G1Jac planes[MSM_SET_POINTS];
  for (uint32_t q = 0; q < MSM_SET_POINTS; q++) {
    planes[q] = pairs[q];
    for (uint32_t s = 1; s < Wb; s++) planes[q] = jac_add(planes[q], pairs[(size_t)MSM_SET_POINTS * s + q]);
  }
  G1Jac acc = msm_set_value(planes, cols);
  // sum_s s * T_s by suffix sums (T_s: the set's plain total, its last point), then "* M" by doublings
  G1Jac run = G1Jac::identity(), weighted = G1Jac::identity();
  for (uint32_t s = Wb - 1; s >= 1; s--) {
    run = jac_add(run, pairs[(size_t)MSM_SET_POINTS * s + MSM_SET_POINTS - 1]);
    weighted = jac_add(weighted, run);
  }
  for (uint32_t l = M; l > 1; l >>= 1) weighted = jac_dbl(weighted);
  return jac_add(acc, weighted);
}

G1Jac msm_fold_windows(const G1Jac* pairs, uint32_t W, uint32_t c, uint32_t cols) {
  G1Jac acc = G1Jac::identity();
  if (c >= 2 && cols == (1u << (c - 1))) {
    // one row of buckets (c <= 8): the row planes are empty, and the Horner over the c - 1 column planes is the low end of
    // the window's own c doublings -- c doublings and c additions per window instead of c + 13 and 15
    for (int w = (int)W - 1; w >= 0; w--) {
      const G1Jac* pl = pairs + (size_t)MSM_SET_POINTS * w;
      acc = jac_dbl(acc);
      for (int t = (int)c - 2; t >= 0; t--) acc = jac_add(jac_dbl(acc), pl[7 + t]);
      acc = jac_add(acc, pl[14]);
    }
    return acc;
  }
  for (int w = (int)W - 1; w >= 0; w--) {
    for (uint32_t j = 0; j < c; j++) acc = jac_dbl(acc);
    acc = jac_add(acc, msm_set_value(pairs + (size_t)MSM_SET_POINTS * w, cols));
  }
  return acc;
}

}  // namespace cq

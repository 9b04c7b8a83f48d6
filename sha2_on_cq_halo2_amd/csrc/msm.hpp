// Internal interface of the G1 MSM engine: msm.hip (launch driver, host folds), msm_sort.hip (sorting fronts), msm_plan.hip (plan scans),
// msm_accumulate.hip (accumulate, combine, reduction, window tables), msm_short.hip (one-kernel short MSM), msm_multi.hip
// (launch planner, table registry); the workspace description is msm_layout.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <optional>
#include <vector>
#include "curve.hpp"
#include "msm_layout.hpp"

struct cq_ctx;

namespace cq {

constexpr uint32_t MSM_ACC_THREADS = 128;

#ifndef CQ_MSM_S1
#define CQ_MSM_S1 24
#endif
constexpr uint32_t MSM_S1 = CQ_MSM_S1;  // max point indices summed by one lane (level 1)
#ifndef CQ_MSM_S1_BIG
#define CQ_MSM_S1_BIG 32
#endif
#ifndef CQ_MSM_S1_BIG_LOAD
#define CQ_MSM_S1_BIG_LOAD 512
#endif
constexpr uint32_t MSM_S1_BIG = CQ_MSM_S1_BIG;  // ... at least this when a bucket expects more than MSM_S1_BIG_LOAD entries
constexpr uint32_t MSM_S1_BIG_LOAD = CQ_MSM_S1_BIG_LOAD;
#ifndef CQ_MSM_PARTIALS_TARGET
#define CQ_MSM_PARTIALS_TARGET 48
#endif
constexpr uint32_t MSM_PARTIALS_TARGET = CQ_MSM_PARTIALS_TARGET;  // partial sums per bucket aimed at under heavy load (< MSM_SHORT)
static_assert(MSM_S1_BIG >= MSM_S1, "the workspace is sized for MSM_S1");
#ifndef CQ_MSM_SMALL_LANES
#define CQ_MSM_SMALL_LANES 65536
#endif
constexpr uint32_t MSM_S1_MIN = 4;
constexpr uint64_t MSM_SMALL_LANES = CQ_MSM_SMALL_LANES;
// (msm_small_launch_s1, the sub-list length of a small launch from its entry bound: msm_layout.hpp)
// sub-lists of a launch whose entry COUNT (known on the device only) is small: at most 65536 x (s1 + 1) / s1 <= 1.25 x 65536
// lanes' worth, plus an MSM that reads another one's lists (counted once more); 3 x 65536 bounds both
constexpr uint64_t MSM_SMALL_PARTIALS = 3 * MSM_SMALL_LANES;
constexpr uint32_t MSM_S2 = 64;         // max partial sums summed by one wave (levels >= 2): one load per lane, six shuffle levels
constexpr uint32_t MSM_SHORT = 64;       // level >= 2 lists up to this long are summed by a lane group when the launch is throughput-bound
constexpr uint32_t MSM_SHORT_MIN = 16;   // ... and lists up to this long always; the ones in between go to a wave each when they are few
#ifndef CQ_MSM_WAVE_BUDGET
#define CQ_MSM_WAVE_BUDGET 4096
#endif
constexpr uint32_t MSM_WAVE_BUDGET = CQ_MSM_WAVE_BUDGET;  // "few": at most this many wave slots in the level (4 per SIMD)
constexpr uint32_t MSM_COMBINE_WAVE_BLOCKS = 2048;  // blocks of the combine levels' wave half (8 192 waves striding over the slots)
constexpr uint32_t MSM_MAX_BATCH = 32;  // MSMs per launch
constexpr uint32_t MSM_SET_POINTS = 15; // points a bucket set leaves for the host: 7 + 7 bit-plane sums and a total (msm_set_value)

// Short plain-mode MSMs (msm_short_run): signed 8-bit windows, one workgroup per (MSM, window).  MSM_SHORT_LIMIT is what the
// kernel is built for (the longest table of the prover's b_by_rows path; a sorted entry has 15 bits of term index, and a term
// takes a byte of LDS); MSM_SHORT_MAX is the cut-over
// of msm_multi_begin, measured against the generic pipeline at batch 8 (profiles/r09_short_msm_ab.txt).
constexpr uint32_t MSM_SHORT_C = 8, MSM_SHORT_W = 32;
constexpr uint32_t MSM_SHORT_LIMIT = 1u << 14;
#ifndef CQ_MSM_SHORT_MAX
#define CQ_MSM_SHORT_MAX 16384
#endif
constexpr uint32_t MSM_SHORT_MAX = CQ_MSM_SHORT_MAX;
static_assert(MSM_SHORT_MAX <= MSM_SHORT_LIMIT && MSM_SHORT_MAX >= 4097, "the cut-over covers N + 1 = 4097 and fits the kernel");

struct MsmPtrs {
  const void* p[MSM_MAX_BATCH];
};
struct MsmStrides {
  uint64_t s[MSM_MAX_BATCH];
};

// The tables a launch's first kernel (msm_set_ptrs_kernel) takes by value and writes to the workspace's pointer table.
// lens: the length the SORT sees (0 for an MSM whose entry lists are another MSM's); src: the MSM whose lists an MSM reads.
struct MsmTableRows {
  MsmPtrs lists, bases;
  MsmStrides strides, lens, src;
};

// Typed view of a launch's workspace: one member per thing the kernels are handed, built from the layout (msm_layout.hpp)
// and the base pointer in ONE place.  Nothing else adds a layout offset to the workspace.
struct MsmBuffers {
  // the pointer table, five rows of `batch` entries (what msm_set_ptrs_kernel writes through `ptrs`)
  const void** ptrs;
  const void* const* lists;      // row 0: the scalars (Fr) -- in index mode the bucket numbers (uint32_t) stand here
  const G1Affine* const* bases;  // row 1
  const uint64_t *strides, *lens, *src;  // rows 2..4
  const Fr* const* scalars() const { return (const Fr* const*)lists; }
  const uint32_t* const* index() const { return (const uint32_t* const*)lists; }
  // counts .. ticket are one span, cleared by the launch's first kernel as `zero_quads` 16-byte stores from `counts`
  uint32_t *counts, *cursor, *ticket;
  size_t zero_quads;
  uint32_t* ranks;  // off_ranks, plain front: one rank per entry.  The partition front cuts the same region in up to four:
  uint32_t *part_pay, *pay2;  // ... payloads of the partition pass and (refinement pass only, else null) of its output
  void* part_low;             // ... the bucket inside the partition: uint8_t, with a refinement pass uint16_t
  uint8_t* low2;              // ... what the refinement pass leaves of it (else null)
  uint32_t *poff, *poff2;     // partition starts of the first pass / of the refinement pass
  uint32_t *psize, *psize2;   // P sizes then P cursors, of the first pass / of the refinement pass
  uint32_t *totals, *index_ticket;  // off_psize again, index front: the lists' entry totals and the count kernel's ticket
  uint32_t* blocksums;        // [nseq][nblk] tile totals of the plan scans ...
  uint32_t* s1_dev;           // ... and, behind them in the same region, the sub-list length the launch settles on
  uint32_t *off /* [nseq][Bt + 1] */, *tk /* [levels][Bt] */, *sorted;
  XYZZ *buckets, *part[2] /* partial sums, ping-pong over the combine levels */, *pairs /* row / column sums */;
  MsmBuffers(const MsmLayout& L, void* workspace);
};

uint32_t msm_window_bits(uint32_t n);
// What one launch of the generic pipeline works on; its shape (n, c, batch, table mode) is the layout's.  Table mode: every
// bases[j] points to a precomputed table [W][stride] with table[w][i] = 2^(c*w)*base[i] (msm_precompute_tables); then there is
// ONE bucket set (or 2^(c-15) of them) per MSM.  by_index (msm_bucket_sums, a table-mode layout): lists[j] holds bucket numbers
// instead of scalars, one entry per point, and the launch ends at the bucket sums (raw_out).
struct MsmLaunch {
  bool by_index;
  const void* const* lists;      // HOST array of `batch` device pointers: Fr scalars; by_index: uint32_t bucket numbers
  const G1Affine* const* bases;  // HOST array of `batch` device pointers
  const size_t* lens;            // per-MSM lengths <= n (one launch may mix lengths); null: n each
  const size_t* strides;         // table mode: table stride per MSM; null: n each (a one-window table)
  G1Jac* window_sums;            // MSM_SET_POINTS points per bucket set -- bit-plane sums the host folds (msm_set_value)
  G1Affine* raw_out;             // by_index: the first raw_count buckets of every MSM, affine; else null
  uint32_t raw_count;
  size_t len(uint32_t i, const MsmLayout& L) const { return lens ? lens[i] : L.n; }
  size_t stride(uint32_t i, const MsmLayout& L) const { return !L.pre ? 0 : strides ? strides[i] : L.n; }
};
// Enqueues the whole pipeline on ctx->stream.  L: the launch's shape; the caller sized `workspace` by it.
int msm_run(cq_ctx* ctx, const MsmLaunch& ln, const MsmLayout& L, void* workspace);

// The stages msm_run enqueues on stream s (msm_sort.hip, msm_plan.hip, msm_accumulate.hip).  s1: the host's sub-list length; any_alias:
// some MSM reads another one's lists.
void msm_enqueue_tables(hipStream_t s, const MsmLayout& L, const MsmBuffers& b, const MsmTableRows& rows);
void msm_plan(hipStream_t s, const MsmLayout& L, const MsmBuffers& b, uint32_t s1, const uint32_t* s1_dev);
void msm_front_plain(hipStream_t s, const MsmLayout& L, const MsmBuffers& b, uint32_t s1);
void msm_front_partition(hipStream_t s, const MsmLayout& L, const MsmBuffers& b, uint32_t s1, bool any_alias);
void msm_front_index(hipStream_t s, const MsmLayout& L, const MsmBuffers& b, uint32_t s1, bool any_alias, uint32_t count);
void msm_accumulate(hipStream_t s, const MsmLayout& L, const MsmBuffers& b);
void msm_combine_levels(hipStream_t s, const MsmLayout& L, const MsmBuffers& b);
void msm_reduce_sets(hipStream_t s, const MsmLayout& L, const MsmBuffers& b, G1Jac* window_sums);
void msm_emit_buckets(hipStream_t s, const MsmLayout& L, const MsmBuffers& b, uint32_t count, G1Affine* out);
// `batch` plain-mode MSMs of n <= MSM_SHORT_LIMIT terms each in ONE kernel on ctx->stream; window_sums_dev as for msm_run with
// c = MSM_SHORT_C (MSM_SHORT_W one-row bucket sets per MSM: the column planes and the total of every set are written);
// workspace: msm_short_workspace(n, batch) bytes
size_t msm_short_workspace(uint32_t n, uint32_t batch);
int msm_short_run(cq_ctx* ctx, const Fr* const* scalars, const G1Affine* const* bases, uint32_t n, uint32_t batch, void* workspace,
                  G1Jac* window_sums_dev);
// Bucket sums instead of an MSM's value: index[j][i] = b < count puts bases29[j][i] into bucket b, any other value
// (0xFFFFFFFF included) nowhere, and out[j][b] = the sum of bucket b, for b < count <= 2^14 -- affine, the callers' R = 2^256
// layout, the identity for a bucket nobody names.  One launch on ctx->stream in a table launch's layout (index front,
// accumulate, combine levels; MSMs with the same index array share their lists); bases29: n points each in the accumulate
// kernel's own form (msm_bases29).
int msm_bucket_sums(cq_ctx* ctx, const uint32_t* const* index, const G1Affine* const* bases29, uint32_t n, uint32_t batch, uint32_t count,
                    G1Affine* out);
// out[i] = bases[i] in the accumulate kernel's packed R' form (window 0 of a table); out == bases converts in place
int msm_bases29(cq_ctx* ctx, const G1Affine* bases, uint32_t n, G1Affine* out);
// can msm_bucket_sums plan a launch of this shape (entry counts below 2^32, workspace within the launches' cap)?
bool msm_bucket_sums_fit(uint32_t n, uint32_t batch);
int msm_precompute_tables(cq_ctx* ctx, const G1Affine* bases, uint32_t n, uint32_t c, G1Affine* table);
// Host: value of one bucket set from its MSM_SET_POINTS points; sum_w 2^(c*w) * (value of set w) over W consecutive sets.
G1Jac msm_set_value(const G1Jac* planes, uint32_t cols);
G1Jac msm_fold_windows(const G1Jac* pairs, uint32_t W, uint32_t c, uint32_t cols);
// Host, table mode with wide windows: the MSM's value from its Wb consecutive sets of M buckets each (set s holds the
// buckets s * M + 1 .. (s + 1) * M):  sum_s ( value(set s) + s * M * total(set s) )
G1Jac msm_fold_sets(const G1Jac* pairs, uint32_t Wb, uint32_t M, uint32_t cols);

}  // namespace cq

// `count` MSMs of equal length, each with its own device base array; Jacobian results on the host
// (count x 12 limbs); one stream synchronisation per launch batch.
int cq_msm_multi(cq_ctx* c, const cq::Fr* const* scalars, const cq::G1Affine* const* bases, size_t len, size_t count,
                 uint64_t* out_jac);
// per-MSM lengths; MSMs over registered (precomputed) bases of any length share launches
int cq_msm_multi_v(cq_ctx* c, const cq::Fr* const* scalars, const cq::G1Affine* const* bases, const size_t* lens, size_t count,
                   uint64_t* out_jac);
// asynchronous form: begin() enqueues every launch and the device->host copy of the results,
// end() waits for the stream and folds them
struct MsmPending {
  struct Launch {
    size_t first = 0, slot = 0;
    uint32_t batch = 0;
    bool empty = false;
    std::optional<cq::MsmLayout> L;  // the launch's shape and workspace (a short launch: the plain c = 8 layout it is folded by); none for an empty one
    bool short_path = false;  // msm_short_run: the result has a plain launch's layout (c = 8), msm_multi_end folds it the same way
  };
  std::vector<Launch> launches;
  void* host = nullptr;
  size_t slots = 0, count = 0;
};
int msm_multi_begin(cq_ctx* c, const cq::Fr* const* scalars, const cq::G1Affine* const* bases, const size_t* lens, size_t count,
                    MsmPending& pend);
int msm_multi_end(cq_ctx* c, MsmPending& pend, uint64_t* out_jac);
// Window width of the precomputed tables: one width per context, so that MSMs over different base arrays can share a
// launch.  15 (17 windows, 2^14 buckets) up to 2^19 terms; wider from 2^20 on, where two or four fewer additions per
// scalar outweigh the larger bucket reduction (msm_table_window_bits; cq_msm_set_table_window overrides).
constexpr uint32_t MSM_TABLE_C = 15, MSM_TABLE_C_MIN = 8, MSM_TABLE_C_MAX = 20;
uint32_t msm_table_window_bits(size_t n);

// Registry of the window tables (msm_multi.hip).  msm_register_tables: makes sure MSMs over [bases, bases + n) find a table --
// of width `want_c` when given, else of the width the array's own length calls for (or the caller's override).  *held
// (optional) tells whether the caller now holds a reference of an entry for exactly (bases, n, width) -- created, or found
// and shared -- that it must give back with msm_release_table; false when the range is served by a larger array's table.
// msm_unregister_tables drops every table of an array that is going away (its owner's call), whoever else held them.
int msm_register_tables(cq_ctx* c, const cq::G1Affine* bases, size_t n, uint32_t want_c = 0, bool* held = nullptr);
void msm_release_table(cq_ctx* c, const void* bases, size_t n, uint32_t c_bits);
void msm_unregister_tables(cq_ctx* c, const void* bases);

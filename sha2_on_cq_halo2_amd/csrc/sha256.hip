// SHA-256 compression circuit: witness synthesis.  The compression chain (64 sequential rounds per block, a few
// microseconds per block) runs on the host and leaves four words per region -- a_r, e_r, W_r and what kind of region it
// is; the kernel below expands them into the 18 advice columns, one thread per row: every cell is a bit field of a word
// that a handful of xors and additions of the region's and its neighbours' (a, e, W) give, placed by the layout table of
// sha256_layout.hpp.  The work is the 18 x n Montgomery encodings and their stores (151 MB at k = 18).
// Wired segments (cq_sha256_synthesize_segments_dev, further down): several chains whose message words may be digest words
// of earlier chains.  There the chains run on the device, one lane per segment and one launch per dependency level, and
// leave the same four words per region for the same expansion kernel.
// Choices (cq_sha256_synthesize_choices_dev): a message word may be one of two operands under a private bit.  The chain
// kernel's fetch takes the operand the bit selects, and a small kernel behind the expansion writes both operands and the
// bit into three cells of the word's region that the layout leaves free.
// Variable length (cq_sha256_synthesize_varlen_dev): raw bytes are padded on the device into the word buffer the plain
// chain kernel reads, and a kernel behind the expansion writes the flags, lengths and selection cells the padding gates read.
// Wired states (cq_sha256_synthesize_states_dev, cq_sha256_synthesize_varlen_from_dev): a segment's chain may start from
// eight gathered words instead of the IV; the chain kernel's INIT instantiations fetch them as they fetch a message word.
// XOR units (cq_sha256_synthesize_xors_dev): a message word may be the XOR of two plain sources.  A small kernel per level
// computes the units that are ready, stores each result behind the segments' digests -- where a message word's fetch finds
// it like a digest word -- and leaves two regions per unit behind the last segment for the same expansion kernel.
#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "cq.hpp"
#include "ctx.hpp"
#include "sha2.hpp"
#include "tablehash.hpp"

namespace cq {

using Sha256 = Sha2Family<uint32_t>;
using Sha256Region = Sha256::Region;

#define SHA256_K_VALUES \
  0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, \
  0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, \
  0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, \
  0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, \
  0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, \
  0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2
static const uint32_t SHA256_K_HOST[64] = {SHA256_K_VALUES};
__constant__ const uint32_t SHA256_K_DEV[64] = {SHA256_K_VALUES};
#define SHA256_IV_VALUES 0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19
static const uint32_t SHA256_IV[8] = {SHA256_IV_VALUES};

__device__ __forceinline__ uint32_t Sha2Family<uint32_t>::k(uint32_t t) { return SHA256_K_DEV[t]; }

// cell I of the layout table, if it sits in row r: the bit field of its word, and the spread form where the cell has one.
// The table entry is a compile-time constant, so `src` and `out` are only ever indexed by constants and stay in registers.
template <uint32_t I>
static __device__ __forceinline__ void sha256_place(const uint32_t (&src)[CQ_SHA256_SRC_COUNT], uint64_t (&out)[CQ_SHA256_ADVICE_COLUMNS],
                                                    uint32_t r, uint32_t table_bits) {
  constexpr Sha256Cell c = SHA256_CELLS[I];
  static_assert(c.kind < CQ_SHA256_SRC_COUNT && c.row < CQ_SHA256_REGION_ROWS, "layout table: word or row out of range");
  static_assert(c.column + (c.form == CQ_SHA256_FORM_PAIR ? 1 : 0) < CQ_SHA256_ADVICE_COLUMNS, "layout table: column out of range");
  if (c.row != r) return;
  const uint32_t off = c.offset + c.per_table_bits * table_bits;
  const uint32_t len = c.len ? c.len : table_bits;
  const uint32_t field = off < 32 ? (src[c.kind] >> off) & (len < 32 ? (1u << len) - 1 : 0xffffffffu) : 0;
  out[c.column] = c.form == CQ_SHA256_FORM_SPREAD ? spread32(field) : field;
  if (c.form == CQ_SHA256_FORM_PAIR) out[c.column + 1] = spread32(field);
}
template <uint32_t... I>
static __device__ __forceinline__ void sha256_place_all(const uint32_t (&src)[CQ_SHA256_SRC_COUNT], uint64_t (&out)[CQ_SHA256_ADVICE_COLUMNS],
                                                        uint32_t r, uint32_t table_bits, std::integer_sequence<uint32_t, I...>) {
  (sha256_place<I>(src, out, r, table_bits), ...);
}

// the row's cell of every column, Montgomery-encoded; a fold over the columns, because a loop the compiler declines to
// unroll would index `out` at run time and send it to scratch memory
template <uint32_t... I>
static __device__ __forceinline__ void sha256_store_all(const Sha2Cols& cols, const uint64_t (&out)[CQ_SHA256_ADVICE_COLUMNS], uint32_t row,
                                                        std::integer_sequence<uint32_t, I...>) {
  (st(cols.p[I] + row, out[I] ? Fr::from_u64(out[I]) : Fr::zero()), ...);
}

// One thread per row.  `regions` holds `nregions` entries; rows behind them are written as zero.
__global__ __launch_bounds__(256) void sha256_expand_kernel(const Sha256Region* __restrict__ regions, uint32_t nregions, uint32_t n,
                                                            uint32_t table_bits, Sha2Cols cols) {
  const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const uint32_t g = row / CQ_SHA256_REGION_ROWS, r = row % CQ_SHA256_REGION_ROWS;
  uint64_t out[CQ_SHA256_ADVICE_COLUMNS];
  CQ_UNROLL for (uint32_t i = 0; i < CQ_SHA256_ADVICE_COLUMNS; i++) out[i] = 0;
  if (g < nregions) {
    uint32_t src[CQ_SHA256_SRC_COUNT];
    sha2_fill_src(src, regions, g);
    sha256_place_all(src, out, r, table_bits, std::make_integer_sequence<uint32_t, SHA256_NUM_CELLS>{});
  }
  sha256_store_all(cols, out, row, std::make_integer_sequence<uint32_t, CQ_SHA256_ADVICE_COLUMNS>{});
}

// the compression chain: the (a, e, W) words and the kind of every region, and the digest
static void sha256_regions(const uint32_t* msg, size_t blocks, std::vector<Sha256Region>& rg, uint32_t digest[8]) {
  uint32_t h[8];
  for (int i = 0; i < 8; i++) h[i] = SHA256_IV[i];
  rg.reserve(blocks * CQ_SHA256_BLOCK_REGIONS + CQ_SHA256_TAIL_REGIONS);
  auto state_regions = [&](bool chained) {  // a_-4 .. a_-1 = d, c, b, a and e_-4 .. e_-1 = h, g, f, e
    for (uint32_t i = 0; i < 4; i++) rg.push_back({h[3 - i], h[7 - i], 0, (chained ? SHA_RG_CHAIN : 0) | (i >= 2 ? SHA_RG_F3 : 0)});
  };
  for (size_t b = 0; b < blocks; b++) {
    state_regions(b > 0);
    uint32_t w[64];
    for (int t = 0; t < 16; t++) w[t] = msg[16 * b + t];
    for (int t = 16; t < 64; t++) w[t] = small_sigma1(w[t - 2]) + w[t - 7] + small_sigma0(w[t - 15]) + w[t - 16];
    uint32_t s[8];
    for (int i = 0; i < 8; i++) s[i] = h[i];
    for (uint32_t t = 0; t < 64; t++) {
      const uint32_t t1 = s[7] + big_sigma1(s[4]) + ch3(s[4], s[5], s[6]) + SHA256_K_HOST[t] + w[t];
      const uint32_t t2 = big_sigma0(s[0]) + maj3(s[0], s[1], s[2]);
      for (int i = 7; i > 0; i--) s[i] = s[i - 1];
      s[4] += t1;
      s[0] = t1 + t2;
      rg.push_back({s[0], s[4], w[t], SHA_RG_ROUND | SHA_RG_F3 | (t >= 16 ? SHA_RG_SCHED : 0) | t << 8});
    }
    for (int i = 0; i < 8; i++) h[i] += s[i];
  }
  state_regions(true);
  for (int i = 0; i < 8; i++) digest[i] = h[i];
}

int sha256_synthesize(cq_ctx* c, uint32_t table_bits, const uint32_t* msg_words, size_t blocks, uint32_t n, const Sha2Cols& cols,
                      uint32_t digest[8]) {
  std::vector<Sha256Region> rg;
  sha256_regions(msg_words, blocks, rg, digest);
  if (rg.size() * CQ_SHA256_REGION_ROWS > n) return c->fail(CQ_ERR_ARG, "sha256: the blocks do not fit the rows");
  static_assert(sizeof(Sha256Region) == 16, "four words per region");
  void* dev;
  int rc = c->ensure_scratch(Scratch::EntryA, rg.size() * sizeof(Sha256Region), &dev);
  if (rc != CQ_OK) return rc;
  CQ_HIP(c, hipMemcpyAsync(dev, rg.data(), rg.size() * sizeof(Sha256Region), hipMemcpyHostToDevice, c->stream));
  CQ_HIP(c, hipStreamSynchronize(c->stream));  // `rg` is pageable and goes away with this call
  sha256_expand_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>((const Sha256Region*)dev, (uint32_t)rg.size(), n, table_bits, cols);
  return hipGetLastError() == hipSuccess ? CQ_OK : c->fail(CQ_ERR_HIP, "sha256_expand launch failed");
}

// ---- wired segments: the compression chains on the device ------------------------------------------------------------

// One entry of the choice table as the device sees it: the bit's index in the word buffer, the two operands (plain
// sources), and -- filled in by the host -- the region of the message word that refers to the entry.
struct Sha256Choice {
  uint32_t bit, zero, one, region;
};

// Message word I of a block.  With CHOICES a source may name an entry of `choices`: the bit and both operands are read and
// the word is `bit ? one : zero`; without, the fetch is a plain source's and `choices` is not looked at.
template <bool CHOICES, uint32_t I>
static __device__ __forceinline__ void sha256_fetch(uint32_t (&w)[16], const uint32_t* src, const Sha256Choice* choices, const uint32_t* words,
                                                    const uint32_t* digests) {
  const uint32_t s = src[I];
  if (CHOICES && !(s & CQ_SHA256_SOURCE_DIGEST) && s >= CQ_SHA256_SOURCE_CHOICE) {
    const uint4 c = *reinterpret_cast<const uint4*>(choices + (s - CQ_SHA256_SOURCE_CHOICE));
    const uint32_t bit = words[c.x], zero = sha2_load(c.y, words, digests), one = sha2_load(c.z, words, digests);
    w[I] = bit ? one : zero;
  } else {
    w[I] = sha2_load(s, words, digests);
  }
}

template <bool CHOICES, uint32_t... I>
static __device__ __forceinline__ void sha256_fetch_all(uint32_t (&w)[16], const uint32_t* src, const Sha256Choice* choices, const uint32_t* words,
                                                        const uint32_t* digests, std::integer_sequence<uint32_t, I...>) {
  (sha256_fetch<CHOICES, I>(w, src, choices, words, digests), ...);
}

// One lane per segment of one level: what sha256_regions does for one message, with the message words gathered through
// `sources`.  A chain is 64 dependent rounds per block, so the launch is latency-bound: one wave per workgroup spreads a
// level's segments over the CUs.  Lanes of a wave may differ in their block counts.  `digests` is read (earlier levels)
// and written (this lane's segment), hence neither const nor restrict.  CHOICES: whether the launch's sources may name
// entries of `choices` (sha256_fetch); a plan without choices runs the instantiation whose fetch knows nothing of them.
// INIT: whether the chains may start from other states than the IV -- `init_sources` then holds 8 entries per segment
// (32 bytes, aligned to 16), each CQ_SHA256_SOURCE_IV or a plain source into `init_words` / `digests`, checked by the
// host like a message word's; lanes of one wave may mix the two.  Without INIT neither pointer is looked at.
template <bool CHOICES, bool INIT>
__global__ __launch_bounds__(64) void sha256_chain_kernel(const Sha2Lane* __restrict__ lanes, uint32_t nlanes,
                                                          const uint32_t* __restrict__ sources, const Sha256Choice* __restrict__ choices,
                                                          const uint32_t* words, uint32_t* digests, Sha256Region* __restrict__ regions,
                                                          const uint32_t* __restrict__ init_sources, const uint32_t* init_words) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nlanes) return;
  const Sha2Lane lane = lanes[i];
  uint32_t h[8] = {SHA256_IV_VALUES};
  if (INIT) sha2_fetch_init_all(h, init_sources + 8 * (size_t)lane.tag, init_words, digests);
  Sha256Region* out = regions + lane.first_region;
  const uint32_t* src = sources + lane.first_source;
  for (uint32_t b = 0; b < lane.blocks; b++, out += CQ_SHA256_BLOCK_REGIONS, src += 16)
    sha2_block(h, out, b ? SHA_RG_CHAIN : 0, [&](uint32_t (&w)[16]) {
      sha256_fetch_all<CHOICES>(w, src, choices, words, digests, std::make_integer_sequence<uint32_t, 16>{});
    });
  sha2_finish(h, out, digests + 8 * (size_t)lane.tag);
}

// the chain launch of one level: the instantiation that knows no more than the description needs
static void sha256_launch_chain(cq_ctx* c, bool choices, bool init, uint32_t grid, const Sha2Lane* lanes, uint32_t nlanes, const uint32_t* sources,
                                const Sha256Choice* dev_choices, const uint32_t* words, uint32_t* digests, Sha256Region* regions,
                                const uint32_t* init_sources, const uint32_t* init_words) {
  if (choices && init)
    sha256_chain_kernel<true, true><<<grid, 64, 0, c->stream>>>(lanes, nlanes, sources, dev_choices, words, digests, regions, init_sources, init_words);
  else if (choices)
    sha256_chain_kernel<true, false><<<grid, 64, 0, c->stream>>>(lanes, nlanes, sources, dev_choices, words, digests, regions, nullptr, nullptr);
  else if (init)
    sha256_chain_kernel<false, true><<<grid, 64, 0, c->stream>>>(lanes, nlanes, sources, nullptr, words, digests, regions, init_sources, init_words);
  else
    sha256_chain_kernel<false, false><<<grid, 64, 0, c->stream>>>(lanes, nlanes, sources, nullptr, words, digests, regions, nullptr, nullptr);
}

// One thread per choice entry, after the expansion (which wrote these cells as zero) on the same stream: the operand taken
// for bit 0, the one taken for bit 1 and the bit word as given, in rows CQ_SHA256_CHOICE_ROW_* of the entry's region in
// column Y.  Every digest is final by now.  The host has checked the entry's indices and set its region, which lies
// below n / CQ_SHA256_REGION_ROWS.
__global__ __launch_bounds__(64) void sha256_choice_fill_kernel(const Sha256Choice* __restrict__ choices, uint32_t nchoices,
                                                                const uint32_t* __restrict__ words, const uint32_t* __restrict__ digests,
                                                                Fr* __restrict__ y) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nchoices) return;
  const uint4 c = *reinterpret_cast<const uint4*>(choices + i);
  const uint32_t bit = words[c.x], zero = sha2_load(c.y, words, digests), one = sha2_load(c.z, words, digests);
  Fr* cell = y + (size_t)c.w * CQ_SHA256_REGION_ROWS;
  st(cell + CQ_SHA256_CHOICE_ROW_ZERO, zero ? Fr::from_u64(zero) : Fr::zero());
  st(cell + CQ_SHA256_CHOICE_ROW_ONE, one ? Fr::from_u64(one) : Fr::zero());
  st(cell + CQ_SHA256_CHOICE_ROW_BIT, bit ? Fr::from_u64(bit) : Fr::zero());
}

// One thread per unit of one level, before the level's chains on the same stream: both operands through sha256_load (the
// digests they may read are earlier levels'), the result word, and the unit's two regions: e = x alone, then e = y with
// W = x ^ y under SHA_RG_F3, whose CHP_EVEN word the expansion computes as this region's e xor the one before.  `digests`
// is read and written, hence neither const nor restrict.  The host has checked every operand against both arrays'
// lengths and that region + 1 lies below n / CQ_SHA256_REGION_ROWS.
__global__ __launch_bounds__(64) void sha256_xor_kernel(const Sha2XorUnit* __restrict__ units, uint32_t nunits, const uint32_t* words,
                                                        uint32_t* digests, Sha256Region* __restrict__ regions) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nunits) return;
  const uint4 u = *reinterpret_cast<const uint4*>(units + i);
  const uint32_t x = sha2_load(u.x, words, digests), y = sha2_load(u.y, words, digests);
  digests[u.z] = x ^ y;
  sha2_put<uint32_t>(regions + u.w, 0, x, 0, 0);
  sha2_put<uint32_t>(regions + u.w + 1, 0, y, x ^ y, SHA_RG_F3);
}

// Validates the description, then queues the tables' upload, one chain launch per level, the expansion and -- with
// choices -- the fill of their cells.  Nothing here waits for the stream; the staging is pinned, and only the previous
// call's copy out of it is waited for.  n_choices = 0 is the description without choices: a source at or above
// CQ_SHA256_SOURCE_CHOICE is then a word index like any other.  init_sources = nullptr is the description whose segments
// all start from the IV; otherwise it holds 8 entries per segment, CQ_SHA256_SOURCE_IV or a plain source.
// n_xors = 0 is the description without XOR units: a digest reference at or above 8 * segments then names a segment that
// does not exist.  Otherwise such a reference in a message word's own source names unit (index - 8 * segments) of `xors`,
// whose result the level's XOR launch stores at that word of `digests_dev` before the chains that read it run.
int sha256_synthesize_segments(cq_ctx* c, uint32_t table_bits, const uint32_t* seg_blocks, size_t segments, const uint32_t* sources,
                               const uint32_t* choices, size_t n_choices, const uint32_t* init_sources, const uint32_t* xors, size_t n_xors,
                               const uint32_t* words_dev, size_t words_len, uint32_t n, const Sha2Cols& cols, uint32_t* digests_dev) {
  uint64_t regions, blocks;
  CQ_TRY(sha2_count_segments<Sha256>(c, seg_blocks, nullptr, segments, n, regions, blocks));
  CQ_TRY(sha2_check_xor_units<Sha256>(c, xors, n_xors, segments, words_len, regions, n));
  std::vector<uint32_t> level(segments, 0);
  std::vector<uint32_t> choice_region(n_choices, UINT32_MAX);  // the region of the word that refers to the entry, once one does
  uint32_t seg_region = 0;
  for (size_t j = 0, at = 0; j < segments; seg_region += seg_blocks[j] * CQ_SHA256_BLOCK_REGIONS + CQ_SHA256_TAIL_REGIONS, j++) {
    for (size_t i = 0; init_sources && i < 8; i++) {  // the state the chain starts from: the IV's word or a plain source
      const uint32_t s = init_sources[8 * j + i];
      if (s == CQ_SHA256_SOURCE_IV) continue;
      const std::string bad = !(s & CQ_SHA256_SOURCE_DIGEST) && n_choices && s >= CQ_SHA256_SOURCE_CHOICE
                                  ? " is a choice, which an initial word cannot be"
                                  : sha2_plain_source(s, j, words_len, level);
      if (!bad.empty()) return c->fail(CQ_ERR_ARG, "sha256: segment " + std::to_string(j) + ", initial word " + std::to_string(i) + bad);
    }
    for (size_t t = 0; t < 16 * (size_t)seg_blocks[j]; t++, at++) {
      auto where = [&] { return "sha256: segment " + std::to_string(j) + ", word " + std::to_string(t); };
      // a plain source, the word's own or a choice's operand: "" if it is good, and the segment's level follows a digest's
      auto plain = [&](uint32_t s) { return sha2_plain_source(s, j, words_len, level); };
      const uint32_t s = sources[at];
      std::string bad;
      if (n_choices && !(s & CQ_SHA256_SOURCE_DIGEST) && s >= CQ_SHA256_SOURCE_CHOICE) {
        const size_t e = s - CQ_SHA256_SOURCE_CHOICE;
        if (e >= n_choices) return c->fail(CQ_ERR_ARG, where() + " reads choice " + std::to_string(e) + " of " + std::to_string(n_choices));
        if (choice_region[e] != UINT32_MAX) return c->fail(CQ_ERR_ARG, where() + " reads choice " + std::to_string(e) + ", which another word reads already");
        choice_region[e] = seg_region + (uint32_t)(t / 16) * CQ_SHA256_BLOCK_REGIONS + 4 + (uint32_t)(t % 16);
        const uint32_t* entry = choices + CQ_SHA256_CHOICE_WORDS * e;
        if (entry[0] >= words_len)
          bad = "'s bit reads word " + std::to_string(entry[0]) + " of a buffer of " + std::to_string(words_len);
        for (uint32_t o = 1; o <= 2 && bad.empty(); o++)
          if (!(bad = plain(entry[o])).empty()) bad = std::string(o == 1 ? "'s zero operand" : "'s one operand") + bad;
        if (!bad.empty()) bad = ", choice " + std::to_string(e) + bad;
      } else if (sha2_reads_xor_unit(s, segments, n_xors)) {
        bad = sha2_xor_reader(s, j, segments, xors, n_xors, words_len, level);
      } else {
        bad = plain(s);
      }
      if (!bad.empty()) return c->fail(CQ_ERR_ARG, where() + bad);
    }
  }
  for (size_t e = 0; e < n_choices; e++)
    if (choice_region[e] == UINT32_MAX) return c->fail(CQ_ERR_ARG, "sha256: choice " + std::to_string(e) + " is read by no word");
  const Sha2Levels lv = sha2_levels(level);
  const std::vector<uint32_t>&level_count = lv.count, &level_first = lv.first;
  const Sha2XorLevels xl = sha2_xor_levels(xors, n_xors, level, level_count.size());
  const std::vector<uint32_t>&xor_count = xl.count, &xor_first = xl.first;

  static_assert(sizeof(Sha256Region) == 16 && sizeof(Sha2Lane) == 16 && sizeof(Sha2XorUnit) == 16, "four words each");
  static_assert(sizeof(Sha256Choice) == CQ_SHA256_CHOICE_WORDS * sizeof(uint32_t), "an entry of the choice table as the header states it");
  // lanes, sources, choices, initial sources, xor units: each a multiple of 16 bytes, so the choice entries, a segment's
  // eight initial sources and the units are aligned for their 16-byte loads
  const size_t lanes_bytes = segments * sizeof(Sha2Lane), sources_bytes = 16 * blocks * sizeof(uint32_t);
  const size_t choices_bytes = n_choices * sizeof(Sha256Choice), init_bytes = init_sources ? 8 * segments * sizeof(uint32_t) : 0;
  const size_t xors_bytes = n_xors * sizeof(Sha2XorUnit);
  const size_t tables_bytes = lanes_bytes + sources_bytes + choices_bytes + init_bytes + xors_bytes;
  const uint64_t all_regions = regions + CQ_SHA256_XOR_REGIONS * (uint64_t)n_xors;  // the units' regions lie behind the last tail
  void *pin, *dev_regions, *dev_tables;
  CQ_TRY(sha2_stage(c, tables_bytes, all_regions * sizeof(Sha256Region), tables_bytes, &pin, &dev_regions, &dev_tables));
  sha2_fill_lanes<Sha256>((Sha2Lane*)pin, seg_blocks, segments, level, lv, [](size_t j) { return (uint32_t)j; });
  memcpy((char*)pin + lanes_bytes, sources, sources_bytes);
  Sha256Choice* staged = (Sha256Choice*)((char*)pin + lanes_bytes + sources_bytes);
  for (size_t e = 0; e < n_choices; e++)
    staged[e] = {choices[CQ_SHA256_CHOICE_WORDS * e], choices[CQ_SHA256_CHOICE_WORDS * e + 1], choices[CQ_SHA256_CHOICE_WORDS * e + 2], choice_region[e]};
  if (init_sources) memcpy((char*)pin + lanes_bytes + sources_bytes + choices_bytes, init_sources, init_bytes);
  sha2_fill_xor_units((Sha2XorUnit*)((char*)pin + lanes_bytes + sources_bytes + choices_bytes + init_bytes), xors, n_xors, xl, segments, regions);
  CQ_TRY(sha2_upload(c, dev_tables, pin, tables_bytes));
  const Sha2Lane* dev_lanes = (const Sha2Lane*)dev_tables;
  const uint32_t* dev_sources = (const uint32_t*)((const char*)dev_tables + lanes_bytes);
  const Sha256Choice* dev_choices = (const Sha256Choice*)((const char*)dev_sources + sources_bytes);
  const uint32_t* dev_init = (const uint32_t*)((const char*)dev_choices + choices_bytes);
  const Sha2XorUnit* dev_units = (const Sha2XorUnit*)((const char*)dev_init + init_bytes);
  auto launch_xors = [&](size_t l) {  // the units that are ready at level l, if there are any
    if (l >= xor_count.size() || !xor_count[l]) return true;
    sha256_xor_kernel<<<(xor_count[l] + 63) / 64, 64, 0, c->stream>>>(dev_units + xor_first[l], xor_count[l], words_dev, digests_dev,
                                                                     (Sha256Region*)dev_regions);
    return hipGetLastError() == hipSuccess;
  };
  for (size_t l = 0; l < level_count.size(); l++) {
    if (!launch_xors(l)) return c->fail(CQ_ERR_HIP, "sha256_xor launch failed");
    sha256_launch_chain(c, n_choices != 0, init_sources != nullptr, (level_count[l] + 63) / 64, dev_lanes + level_first[l], level_count[l],
                        dev_sources, dev_choices, words_dev, digests_dev, (Sha256Region*)dev_regions, dev_init, words_dev);
    if (hipGetLastError() != hipSuccess) return c->fail(CQ_ERR_HIP, "sha256_chain launch failed");
  }
  if (!launch_xors(level_count.size())) return c->fail(CQ_ERR_HIP, "sha256_xor launch failed");  // units over the last level's digests
  sha256_expand_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>((const Sha256Region*)dev_regions, (uint32_t)all_regions, n, table_bits, cols);
  if (hipGetLastError() != hipSuccess) return c->fail(CQ_ERR_HIP, "sha256_expand launch failed");
  if (n_choices) {
    sha256_choice_fill_kernel<<<((uint32_t)n_choices + 63) / 64, 64, 0, c->stream>>>(dev_choices, (uint32_t)n_choices, words_dev, digests_dev,
                                                                                    cols.p[SHA256_COL_Y]);
    if (hipGetLastError() != hipSuccess) return c->fail(CQ_ERR_HIP, "sha256_choice_fill launch failed");
  }
  return CQ_OK;
}

// ---- messages of variable length: padding on the device, and the cells its gates read --------------------------------

// One message of a variable-length synthesis: where its raw bytes start in the caller's buffer, how many there are, and
// the bytes absorbed before them (a multiple of 64; zero unless the chain continues from a state).
struct Sha256VarMsg {
  uint64_t offset;
  uint32_t len, base;
};

// The segment that holds word `word` of the word buffer: lanes are in segment order there and lane j's words start at
// first_source, ascending, lane 0's at 0; `word` lies below the buffer's end.
static __device__ __forceinline__ uint32_t sha256_var_segment(const Sha2Lane* __restrict__ lanes, uint32_t nlanes, uint32_t word) {
  uint32_t lo = 0, hi = nlanes;  // lanes[lo].first_source <= word < lanes[hi].first_source (hi = nlanes: the end)
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (lanes[mid].first_source <= word) lo = mid; else hi = mid;
  }
  return lo;
}

// the index of a message's final block: the first with room for 0x80 and the 64-bit length behind the data
static SHA_HD uint32_t sha256_var_final_block(uint32_t len) { return (len + 8) / 64; }

// One thread per word of the word buffer (16 per block of every segment, segment after segment): the big-endian word of
// the padded message -- data bytes, 0x80, zeros, the bit length of base + len bytes in word 15 of the final block (the
// host has checked that it is a 32-bit word) -- and zero behind the final block.  A byte is loaded only below the message's length, which the host has checked against the buffer.
__global__ __launch_bounds__(256) void sha256_pad_kernel(const Sha2Lane* __restrict__ lanes, const Sha256VarMsg* __restrict__ msgs,
                                                         uint32_t nlanes, uint32_t nwords, const uint8_t* __restrict__ bytes,
                                                         uint32_t* __restrict__ words) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nwords) return;
  const uint32_t j = sha256_var_segment(lanes, nlanes, i);
  const uint32_t t = i - lanes[j].first_source, len = msgs[j].len, last = 16 * sha256_var_final_block(len) + 15;
  const uint8_t* src = bytes + msgs[j].offset;
  uint32_t w = 0;
  if (t == last) {
    w = 8 * (msgs[j].base + len);
  } else if (t < last) {
    CQ_UNROLL for (uint32_t k = 0; k < 4; k++) {
      const uint32_t pos = 4 * t + k;
      const uint32_t byte = pos < len ? src[pos] : (pos == len ? 0x80u : 0u);
      w |= byte << (24 - 8 * k);
    }
  }
  words[i] = w;
}

static __device__ __forceinline__ void sha256_var_put(Fr* cell, uint64_t v) { st(cell, v ? Fr::from_u64(v) : Fr::zero()); }

// The flag and the running length of word g (16 * block + word) of a message of `len` bytes whose final block is `fb`:
// the word lies wholly inside the message; the bytes of the message up to and with the word -- zero behind the final block,
// where the length a block starts from is cleared.  The length counts from `base`, the bytes absorbed before the message.
static __device__ __forceinline__ uint32_t sha256_var_m(uint32_t g, uint32_t len) { return 4 * (g + 1) <= len ? 1u : 0u; }
static __device__ __forceinline__ uint32_t sha256_var_len(uint32_t g, uint32_t len, uint32_t fb, uint32_t base) {
  return g / 16 > fb ? 0u : base + min(4 * (g + 1), len);
}

// 32 threads per block of every segment, after the expansion (which wrote these cells as zero) on the same stream; a
// thread's role is its index among the 32.  0 .. 15: the message-word region of that word -- flag, length, and in the
// boundary word the two bits, their product and the halves of its data bytes.  16: the block's carry-in region.
// 17 .. 24: the region that adds digest word (role - 17) of the chaining value behind the block, if the block is final,
// to the word selected so far; the last block's sum goes to `digests`, over the chain kernel's digest.  25: the final
// flag.  26: the same sum for the length.  The host has checked that every region of every lane lies below
// n / CQ_SHA256_REGION_ROWS; `regions` is what the chain kernel left.
__global__ __launch_bounds__(256) void sha256_varlen_fill_kernel(const Sha2Lane* __restrict__ lanes, const Sha256VarMsg* __restrict__ msgs,
                                                                 uint32_t nlanes, uint32_t nblocks, const Sha256Region* __restrict__ regions,
                                                                 Sha2Cols cols, uint32_t* __restrict__ digests) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t gb = i / 32, role = i % 32;
  if (gb >= nblocks || role > 26) return;
  const uint32_t j = sha256_var_segment(lanes, nlanes, 16 * gb);
  const Sha2Lane lane = lanes[j];
  const uint32_t b = gb - lane.first_source / 16, len = msgs[j].len, base = msgs[j].base, fb = sha256_var_final_block(len);
  const uint32_t block_region = lane.first_region + b * CQ_SHA256_BLOCK_REGIONS;
  Fr* const y = cols.p[SHA256_COL_Y];
  const uint32_t m13_before = b ? sha256_var_m(16 * b - 3, len) : 1u, m13 = sha256_var_m(16 * b + 13, len);
  if (role < 16) {
    const uint32_t g = 16 * b + role;
    const size_t row = (size_t)(block_region + 4 + role) * CQ_SHA256_REGION_ROWS;
    sha256_var_put(y + row + CQ_SHA256_VAR_ROW_M, sha256_var_m(g, len));
    sha256_var_put(y + row + CQ_SHA256_VAR_ROW_LEN, sha256_var_len(g, len, fb, base));
    if (g == len / 4) {  // the boundary word: r = len % 4 bytes of the message, 0x80, zeros
      const uint32_t r = len % 4, s = 3 - r, c0 = s & 1, c1 = s >> 1;
      const uint32_t data = r ? regions[block_region + 4 + role].w >> (32 - 8 * r) : 0;
      const uint32_t d0 = data & 0xfffu, d1 = data >> 12;
      sha256_var_put(y + row + CQ_SHA256_VAR_ROW_C0, c0);
      sha256_var_put(y + row + CQ_SHA256_VAR_ROW_C1, c1);
      sha256_var_put(cols.p[2 * CQ_SHA256_VAR_SLOT_PRODUCT] + row, c0 & c1);  // a bit is its own spread form
      sha256_var_put(cols.p[2 * CQ_SHA256_VAR_SLOT_PRODUCT + 1] + row, c0 & c1);
      sha256_var_put(cols.p[2 * CQ_SHA256_VAR_SLOT_DATA] + row, d0);
      sha256_var_put(cols.p[2 * CQ_SHA256_VAR_SLOT_DATA + 1] + row, spread32(d0));
      sha256_var_put(cols.p[2 * CQ_SHA256_VAR_SLOT_DATA] + row + 1, d1);
      sha256_var_put(cols.p[2 * CQ_SHA256_VAR_SLOT_DATA + 1] + row + 1, spread32(d1));
    }
  } else if (role == 16) {
    const size_t row = (size_t)(block_region + CQ_SHA256_VAR_REGION_CARRY) * CQ_SHA256_REGION_ROWS;
    const uint32_t len15 = b ? sha256_var_len(16 * b - 1, len, fb, base) : 0u;
    sha256_var_put(y + row + CQ_SHA256_VAR_ROW_M, b ? sha256_var_m(16 * b - 1, len) : 1u);
    sha256_var_put(y + row + CQ_SHA256_VAR_ROW_LEN, b ? len15 * m13_before : base);
    sha256_var_put(y + row + CQ_SHA256_VAR_ROW_VALUE, len15);
    sha256_var_put(y + row + CQ_SHA256_VAR_ROW_OUT, b ? m13_before : 0u);
  } else if (role == 25) {
    const size_t row = (size_t)(block_region + CQ_SHA256_VAR_REGION_FINAL) * CQ_SHA256_REGION_ROWS;
    sha256_var_put(y + row + CQ_SHA256_VAR_ROW_IN, m13_before);
    sha256_var_put(y + row + CQ_SHA256_VAR_ROW_FLAG, m13);
    sha256_var_put(y + row + CQ_SHA256_VAR_ROW_VALUE, m13_before - m13);
  } else {
    // digest word w of the chaining value behind block c: state region 3 - w % 4 of block c + 1 (or of the tail)
    auto chaining = [&](uint32_t c, uint32_t w) {
      const Sha256Region h = regions[lane.first_region + (c + 1) * CQ_SHA256_BLOCK_REGIONS + 3 - w % 4];
      return w < 4 ? h.a : h.e;
    };
    const bool is_len = role == 26;
    const uint32_t w = role - 17;
    const size_t row = (size_t)(block_region + (is_len ? CQ_SHA256_VAR_REGION_LENGTH : CQ_SHA256_VAR_REGION_SUM + w)) * CQ_SHA256_REGION_ROWS;
    // the final block lies inside the lane (the host has checked the length against the block count)
    const uint32_t selected = is_len ? base + len : chaining(fb, w);
    const uint32_t out = b >= fb ? selected : 0u;
    sha256_var_put(y + row + CQ_SHA256_VAR_ROW_IN, b > fb ? selected : 0u);
    sha256_var_put(y + row + CQ_SHA256_VAR_ROW_FLAG, b == fb ? 1u : 0u);
    sha256_var_put(y + row + CQ_SHA256_VAR_ROW_VALUE, is_len ? sha256_var_len(16 * b + 15, len, fb, base) : chaining(b, w));
    sha256_var_put(y + row + CQ_SHA256_VAR_ROW_OUT, out);
    if (!is_len && b + 1 == lane.blocks) digests[8 * (size_t)lane.tag + w] = out;
  }
}

// Validates the messages against their segments, the buffer and the rows, then queues: the upload of the lane, message and
// source tables (pinned staging, as sha256_synthesize_segments), the padding into the word buffer, one launch of the plain
// chain kernel over all segments (a padded message reads no digest: every segment has level 0, and its sources are its own
// words in order), the expansion, and the fill of the padding gates' cells.  Nothing here waits for the stream.
// init_states_dev = nullptr: every chain starts from the IV after no byte.  Otherwise segment j starts from the eight words
// at init_states_dev + 8 j after base_lens[j] bytes: the chain launch is the INIT instantiation with the identity for its
// initial sources, which rides behind the word sources in the same upload.
int sha256_synthesize_varlen(cq_ctx* c, uint32_t table_bits, const uint32_t* seg_max_blocks, size_t segments, const uint8_t* bytes_dev,
                             size_t bytes_len, const uint64_t* offsets, const uint64_t* lens, const uint32_t* init_states_dev,
                             const uint64_t* base_lens, uint32_t n, const Sha2Cols& cols, uint32_t* digests_dev) {
  uint64_t regions, blocks;
  CQ_TRY(sha2_count_segments<Sha256>(c, seg_max_blocks, nullptr, segments, n, regions, blocks, [&](size_t j) {
    auto seg = [&] { return "sha256: segment " + std::to_string(j); };
    // n < 2^31 bounds the blocks, so 64 * blocks stays far below 2^29 and 8 * length is a 32-bit word
    if (lens[j] > 64 * (uint64_t)seg_max_blocks[j] - 9)
      return c->fail(CQ_ERR_ARG, seg() + ": a message of " + std::to_string(lens[j]) + " bytes does not pad to " +
                                     std::to_string(seg_max_blocks[j]) + " blocks or fewer");
    if (offsets[j] > bytes_len || lens[j] > bytes_len - offsets[j])
      return c->fail(CQ_ERR_ARG, seg() + ": bytes " + std::to_string(offsets[j]) + " .. " + std::to_string(offsets[j]) + " + " +
                                     std::to_string(lens[j]) + " leave a buffer of " + std::to_string(bytes_len));
    // the bit length of base + length is the 32-bit word 15 of the final block: the total stays below 2^29 bytes
    if (base_lens && base_lens[j] % 64)
      return c->fail(CQ_ERR_ARG, seg() + ": a base of " + std::to_string(base_lens[j]) + " bytes is no multiple of 64");
    if (base_lens && (base_lens[j] > (1ull << 29) || base_lens[j] + 64 * (uint64_t)seg_max_blocks[j] > (1ull << 29)))
      return c->fail(CQ_ERR_ARG, seg() + ": a base of " + std::to_string(base_lens[j]) + " bytes and " + std::to_string(seg_max_blocks[j]) +
                                     " blocks reach past 2^29 bytes");
    return (int)CQ_OK;
  }));
  static_assert(sizeof(Sha256VarMsg) == 16, "four words");
  const size_t lanes_bytes = segments * sizeof(Sha2Lane), msgs_bytes = segments * sizeof(Sha256VarMsg);
  const size_t nwords = 16 * blocks, words_bytes = nwords * sizeof(uint32_t);
  const size_t init_bytes = init_states_dev ? 8 * segments * sizeof(uint32_t) : 0;
  // the sources: one index per word; each part a multiple of 16 bytes
  const size_t tables_bytes = lanes_bytes + msgs_bytes + words_bytes + init_bytes;
  void *pin, *dev_regions, *dev_tables;
  CQ_TRY(sha2_stage(c, tables_bytes, regions * sizeof(Sha256Region), tables_bytes + words_bytes, &pin, &dev_regions,
                    &dev_tables));  // behind the tables: the word buffer
  Sha2Lane* lanes = (Sha2Lane*)pin;
  Sha256VarMsg* msgs = (Sha256VarMsg*)((char*)pin + lanes_bytes);
  uint32_t* sources = (uint32_t*)((char*)pin + lanes_bytes + msgs_bytes);
  sha2_fill_lanes<Sha256>(lanes, seg_max_blocks, segments, {}, {}, [](size_t j) { return (uint32_t)j; });
  for (size_t j = 0; j < segments; j++) msgs[j] = {offsets[j], (uint32_t)lens[j], base_lens ? (uint32_t)base_lens[j] : 0u};
  for (size_t i = 0; i < nwords; i++) sources[i] = (uint32_t)i;
  for (size_t i = 0; i < init_bytes / sizeof(uint32_t); i++) sources[nwords + i] = (uint32_t)i;
  CQ_TRY(sha2_upload(c, dev_tables, pin, tables_bytes));
  const Sha2Lane* dev_lanes = (const Sha2Lane*)dev_tables;
  const Sha256VarMsg* dev_msgs = (const Sha256VarMsg*)((const char*)dev_tables + lanes_bytes);
  const uint32_t* dev_sources = (const uint32_t*)((const char*)dev_msgs + msgs_bytes);
  uint32_t* dev_words = (uint32_t*)((char*)dev_tables + tables_bytes);
  sha256_pad_kernel<<<((uint32_t)nwords + 255) / 256, 256, 0, c->stream>>>(dev_lanes, dev_msgs, (uint32_t)segments, (uint32_t)nwords, bytes_dev,
                                                                          dev_words);
  if (hipGetLastError() != hipSuccess) return c->fail(CQ_ERR_HIP, "sha256_pad launch failed");
  sha256_launch_chain(c, false, init_states_dev != nullptr, ((uint32_t)segments + 63) / 64, dev_lanes, (uint32_t)segments, dev_sources, nullptr,
                      dev_words, digests_dev, (Sha256Region*)dev_regions, dev_sources + nwords, init_states_dev);
  if (hipGetLastError() != hipSuccess) return c->fail(CQ_ERR_HIP, "sha256_chain launch failed");
  sha256_expand_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>((const Sha256Region*)dev_regions, (uint32_t)regions, n, table_bits, cols);
  if (hipGetLastError() != hipSuccess) return c->fail(CQ_ERR_HIP, "sha256_expand launch failed");
  sha256_varlen_fill_kernel<<<(uint32_t)((32 * blocks + 255) / 256), 256, 0, c->stream>>>(dev_lanes, dev_msgs, (uint32_t)segments, (uint32_t)blocks,
                                                                                         (const Sha256Region*)dev_regions, cols, digests_dev);
  if (hipGetLastError() != hipSuccess) return c->fail(CQ_ERR_HIP, "sha256_varlen_fill launch failed");
  return CQ_OK;
}

}  // namespace cq

using namespace cq;

extern "C" {

int cq_sha256_layout(uint32_t* cells, size_t cap, size_t* count) {
  if (!count || (cap && !cells)) return CQ_ERR_ARG;
  *count = SHA256_NUM_CELLS;
  for (size_t i = 0; i < cap && i < SHA256_NUM_CELLS; i++) {
    const Sha256Cell& s = SHA256_CELLS[i];
    const uint32_t words[CQ_SHA256_CELL_WORDS] = {s.kind, s.form, s.column, s.row, s.offset, s.per_table_bits, s.len};
    for (uint32_t j = 0; j < CQ_SHA256_CELL_WORDS; j++) cells[i * CQ_SHA256_CELL_WORDS + j] = words[j];
  }
  return CQ_OK;
}

int cq_sha256_synthesize_dev(cq_ctx* c, uint32_t table_bits, const uint32_t* msg_words, size_t blocks, size_t n,
                             uint64_t* const* cols_dev, uint32_t digest[8]) {
  if (!c || !msg_words || !cols_dev || !digest || blocks == 0 || n > 0x7fffffffull || blocks > n) return CQ_ERR_ARG;
  Sha2Cols sc;
  CQ_TRY(sha2_entry(c, "sha256", nullptr, table_bits, CQ_SHA256_MIN_TABLE_BITS, CQ_SHA256_MAX_TABLE_BITS, "the pieces", cols_dev, sc));
  return sha256_synthesize(c, table_bits, msg_words, blocks, (uint32_t)n, sc, digest);
}

// the four entry points below: the argument checks that need no description, then the host function
static int sha256_segments_entry(cq_ctx* c, uint32_t table_bits, const uint32_t* seg_blocks, size_t segments, const uint32_t* sources,
                                 const uint32_t* choices, size_t n_choices, const uint32_t* init_sources, const uint32_t* xors, size_t n_xors,
                                 const uint32_t* words_dev, size_t words_len, size_t n, uint64_t* const* cols_dev, uint32_t* digests_dev) {
  if (!c) return CQ_ERR_ARG;
  const char* bad = nullptr;
  if (!seg_blocks || !sources || !cols_dev || !digests_dev || segments == 0 || n > 0x7fffffffull || (!words_dev && words_len) ||
      words_len > CQ_SHA256_SOURCE_DIGEST)
    bad = SHA2_BAD_ARGS;
  else if (n_choices && (!choices || words_len > CQ_SHA256_SOURCE_CHOICE || n_choices > n))
    bad = "null choice table, more choices than rows, or a word buffer that reaches the choice flag";
  else if (n_xors && (!xors || n_xors > n))
    bad = "null xor table, or more xor units than rows";
  Sha2Cols sc;
  CQ_TRY(sha2_entry(c, "sha256", bad, table_bits, CQ_SHA256_MIN_TABLE_BITS, CQ_SHA256_MAX_TABLE_BITS, "the pieces", cols_dev, sc));
  return sha256_synthesize_segments(c, table_bits, seg_blocks, segments, sources, choices, n_choices, init_sources, xors, n_xors, words_dev,
                                    words_len, (uint32_t)n, sc, digests_dev);
}

int cq_sha256_synthesize_segments_dev(cq_ctx* c, uint32_t table_bits, const uint32_t* seg_blocks, size_t segments,
                                      const uint32_t* sources, const uint32_t* words_dev, size_t words_len, size_t n,
                                      uint64_t* const* cols_dev, uint32_t* digests_dev) {
  return sha256_segments_entry(c, table_bits, seg_blocks, segments, sources, nullptr, 0, nullptr, nullptr, 0, words_dev, words_len, n, cols_dev,
                               digests_dev);
}

int cq_sha256_synthesize_choices_dev(cq_ctx* c, uint32_t table_bits, const uint32_t* seg_blocks, size_t segments,
                                     const uint32_t* sources, const uint32_t* choices, size_t n_choices, const uint32_t* words_dev,
                                     size_t words_len, size_t n, uint64_t* const* cols_dev, uint32_t* digests_dev) {
  return sha256_segments_entry(c, table_bits, seg_blocks, segments, sources, choices, n_choices, nullptr, nullptr, 0, words_dev, words_len, n,
                               cols_dev, digests_dev);
}

int cq_sha256_synthesize_states_dev(cq_ctx* c, uint32_t table_bits, const uint32_t* seg_blocks, size_t segments,
                                    const uint32_t* sources, const uint32_t* choices, size_t n_choices, const uint32_t* init_sources,
                                    const uint32_t* words_dev, size_t words_len, size_t n, uint64_t* const* cols_dev,
                                    uint32_t* digests_dev) {
  return sha256_segments_entry(c, table_bits, seg_blocks, segments, sources, choices, n_choices, init_sources, nullptr, 0, words_dev, words_len, n,
                               cols_dev, digests_dev);
}

int cq_sha256_synthesize_xors_dev(cq_ctx* c, uint32_t table_bits, const uint32_t* seg_blocks, size_t segments, const uint32_t* sources,
                                  const uint32_t* choices, size_t n_choices, const uint32_t* init_sources, const uint32_t* xors,
                                  size_t n_xors, const uint32_t* words_dev, size_t words_len, size_t n, uint64_t* const* cols_dev,
                                  uint32_t* digests_dev) {
  return sha256_segments_entry(c, table_bits, seg_blocks, segments, sources, choices, n_choices, init_sources, xors, n_xors, words_dev, words_len,
                               n, cols_dev, digests_dev);
}

// both entry points below: the argument checks that need no message, then the host function
static int sha256_varlen_entry(cq_ctx* c, uint32_t table_bits, const uint32_t* seg_max_blocks, size_t segments, const uint8_t* msg_bytes_dev,
                               size_t msg_bytes_len, const uint64_t* msg_offsets, const uint64_t* msg_lens, const uint32_t* init_states_dev,
                               const uint64_t* base_lens, size_t n, uint64_t* const* cols_dev, uint32_t* digests_dev) {
  if (!c) return CQ_ERR_ARG;
  const bool bad = !seg_max_blocks || !msg_offsets || !msg_lens || !cols_dev || !digests_dev || segments == 0 || n > 0x7fffffffull ||
                   (!msg_bytes_dev && msg_bytes_len);
  Sha2Cols sc;
  CQ_TRY(sha2_entry(c, "sha256", bad ? SHA2_BAD_ARGS : nullptr, table_bits, CQ_SHA256_VAR_MIN_TABLE_BITS, CQ_SHA256_MAX_TABLE_BITS,
                    "the 12-bit halves of a boundary word's bytes", cols_dev, sc));
  return sha256_synthesize_varlen(c, table_bits, seg_max_blocks, segments, msg_bytes_dev, msg_bytes_len, msg_offsets, msg_lens, init_states_dev,
                                  base_lens, (uint32_t)n, sc, digests_dev);
}

int cq_sha256_synthesize_varlen_dev(cq_ctx* c, uint32_t table_bits, const uint32_t* seg_max_blocks, size_t segments,
                                    const uint8_t* msg_bytes_dev, size_t msg_bytes_len, const uint64_t* msg_offsets,
                                    const uint64_t* msg_lens, size_t n, uint64_t* const* cols_dev, uint32_t* digests_dev) {
  return sha256_varlen_entry(c, table_bits, seg_max_blocks, segments, msg_bytes_dev, msg_bytes_len, msg_offsets, msg_lens, nullptr, nullptr, n,
                             cols_dev, digests_dev);
}

int cq_sha256_synthesize_varlen_from_dev(cq_ctx* c, uint32_t table_bits, const uint32_t* seg_max_blocks, size_t segments,
                                         const uint8_t* msg_bytes_dev, size_t msg_bytes_len, const uint64_t* msg_offsets,
                                         const uint64_t* msg_lens, const uint32_t* init_states_dev, const uint64_t* base_lens, size_t n,
                                         uint64_t* const* cols_dev, uint32_t* digests_dev) {
  if (c && (!init_states_dev || !base_lens)) return c->fail(CQ_ERR_ARG, "sha256: null initial states or base lengths");
  return sha256_varlen_entry(c, table_bits, seg_max_blocks, segments, msg_bytes_dev, msg_bytes_len, msg_offsets, msg_lens, init_states_dev,
                             base_lens, n, cols_dev, digests_dev);
}

}  // extern "C"

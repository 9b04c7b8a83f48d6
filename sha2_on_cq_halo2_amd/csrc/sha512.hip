// SHA-512 / SHA-384 compression circuit: witness synthesis.  The 64-bit counterpart of sha256.hip's segment path without
// wiring: every segment is an independent message, so one launch runs all the compression chains, one lane per segment
// (80 sequential rounds per 128-byte block), and leaves four 64-bit words per region on the device -- a_r, e_r, W_r and
// what kind of region it is.  The expansion kernel turns them into the 18 advice columns, one thread per row: every cell
// is a bit field of a word that a handful of xors and additions of the region's and its neighbours' (a, e, W) give,
// placed by the layout table of sha512_layout.hpp.  The spread form of a 64-bit word has 128 bits, so a cell value is two
// 64-bit limbs until it is Montgomery-encoded.
// XOR units (cq_sha512_synthesize_xors_dev): a message word may be the XOR of two plain sources, as in sha256.hip.  A small
// kernel per level computes the units that are ready, stores each result behind the segments' digests -- where a message
// word's fetch finds it like a digest word -- and leaves two regions per unit behind the last segment for the same
// expansion kernel.
#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "cq.hpp"
#include "ctx.hpp"
#include "sha2.hpp"
#include "sha512_layout.hpp"
#include "tablehash.hpp"

namespace cq {

using Sha512 = Sha2Family<uint64_t>;
using Sha512Region = Sha512::Region;

__constant__ const uint64_t SHA512_K_DEV[80] = {
    0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull, 0x59f111f1b605d019ull,
    0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
    0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull,
    0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull, 0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
    0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
    0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
    0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull, 0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull,
    0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
    0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull,
    0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
    0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull, 0xd186b8c721c0c207ull,
    0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
    0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull,
    0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
// the initial hash values by CQ_SHA512_VARIANT_*
__constant__ const uint64_t SHA512_IV_DEV[2][8] = {
    {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full,
     0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull},
    {0xcbbb9d5dc1059ed8ull, 0x629a292a367cd507ull, 0x9159015a3070dd17ull, 0x152fecd8f70e5939ull, 0x67332667ffc00b31ull, 0x8eb44a8768581511ull,
     0xdb0c2e0d64f98fa7ull, 0x47b5481dbefa4fa4ull}};
static_assert(CQ_SHA512_VARIANT_512 == 0 && CQ_SHA512_VARIANT_384 == 1, "the rows of SHA512_IV_DEV");

__device__ __forceinline__ uint64_t Sha2Family<uint64_t>::k(uint32_t t) { return SHA512_K_DEV[t]; }

// a cell value below 2^128 -> Montgomery form
static SHA_D Fr sha512_encode(uint64_t lo, uint64_t hi) {
  const uint64_t limbs[4] = {lo, hi, 0, 0};
  return Fr::from_limbs64(limbs) * Fr::r2();
}

// cell I of the layout table, if it sits in row r: the bit field of its word, and the spread form where the cell has one.
// The table entry is a compile-time constant, so `src`, `lo` and `hi` are only ever indexed by constants and stay in
// registers.  A chunk may start at or above bit 64 (table_bits 13 and wider) and a word cell has all 64 bits: neither
// shift below is ever by 64 or more.  A pair cell's field has at most CQ_SHA512_MAX_TABLE_BITS = 16 bits, so its spread
// form is one 32-bit spread; only a word's spread form fills the high limb.
template <uint32_t I>
static SHA_D void sha512_place(const uint64_t (&src)[CQ_SHA256_SRC_COUNT], uint64_t (&lo)[CQ_SHA256_ADVICE_COLUMNS],
                               uint64_t (&hi)[CQ_SHA256_ADVICE_COLUMNS], uint32_t r, uint32_t table_bits) {
  constexpr Sha256Cell c = SHA512_CELLS[I];
  static_assert(c.kind < CQ_SHA256_SRC_COUNT && c.row < CQ_SHA512_REGION_ROWS, "layout table: word or row out of range");
  static_assert(c.column + (c.form == CQ_SHA256_FORM_PAIR ? 1 : 0) < CQ_SHA256_ADVICE_COLUMNS, "layout table: column out of range");
  static_assert(c.form == CQ_SHA256_FORM_PAIR ? c.len <= CQ_SHA512_MIN_TABLE_BITS && c.offset + c.len <= 64 : c.len == 64 && c.offset == 0,
                "layout table: a piece wider than the smallest table, or a word cell that is not the whole word");
  static_assert(CQ_SHA512_MAX_TABLE_BITS <= 16, "a pair cell's spread form is a 32-bit spread");
  if (c.row != r) return;
  if constexpr (c.form == CQ_SHA256_FORM_PAIR) {
    const uint32_t off = c.offset + c.per_table_bits * table_bits;
    const uint32_t len = c.len ? c.len : table_bits;
    const uint32_t field = off < 64 ? (uint32_t)(src[c.kind] >> off) & ((1u << len) - 1) : 0u;
    lo[c.column] = field;
    lo[c.column + 1] = spread32(field);
  } else if constexpr (c.form == CQ_SHA256_FORM_SPREAD) {
    lo[c.column] = spread32((uint32_t)src[c.kind]);
    hi[c.column] = spread32((uint32_t)(src[c.kind] >> 32));
  } else {
    lo[c.column] = src[c.kind];
  }
}
template <uint32_t... I>
static SHA_D void sha512_place_all(const uint64_t (&src)[CQ_SHA256_SRC_COUNT], uint64_t (&lo)[CQ_SHA256_ADVICE_COLUMNS],
                                   uint64_t (&hi)[CQ_SHA256_ADVICE_COLUMNS], uint32_t r, uint32_t table_bits,
                                   std::integer_sequence<uint32_t, I...>) {
  (sha512_place<I>(src, lo, hi, r, table_bits), ...);
}

// the row's cell of every column, Montgomery-encoded; a fold over the columns, because a loop the compiler declines to
// unroll would index `lo` and `hi` at run time and send them to scratch memory
template <uint32_t... I>
static SHA_D void sha512_store_all(const Sha2Cols& cols, const uint64_t (&lo)[CQ_SHA256_ADVICE_COLUMNS],
                                   const uint64_t (&hi)[CQ_SHA256_ADVICE_COLUMNS], uint32_t row, std::integer_sequence<uint32_t, I...>) {
  (st(cols.p[I] + row, (lo[I] | hi[I]) ? sha512_encode(lo[I], hi[I]) : Fr::zero()), ...);
}

// One thread per row.  `regions` holds `nregions` entries; rows behind them are written as zero, rows at or behind n not
// at all.
__global__ __launch_bounds__(256) void sha512_expand_kernel(const Sha512Region* __restrict__ regions, uint32_t nregions, uint32_t n,
                                                            uint32_t table_bits, Sha2Cols cols) {
  const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const uint32_t g = row / CQ_SHA512_REGION_ROWS, r = row % CQ_SHA512_REGION_ROWS;
  uint64_t lo[CQ_SHA256_ADVICE_COLUMNS], hi[CQ_SHA256_ADVICE_COLUMNS];
  CQ_UNROLL for (uint32_t i = 0; i < CQ_SHA256_ADVICE_COLUMNS; i++) lo[i] = hi[i] = 0;
  if (g < nregions) {
    uint64_t src[CQ_SHA256_SRC_COUNT];
    sha2_fill_src(src, regions, g);
    sha512_place_all(src, lo, hi, r, table_bits, std::make_integer_sequence<uint32_t, SHA512_NUM_CELLS>{});
  }
  sha512_store_all(cols, lo, hi, row, std::make_integer_sequence<uint32_t, CQ_SHA256_ADVICE_COLUMNS>{});
}

// The 16 message words of a block.  Unwired, `words` points at them; WIRED, `src` holds their 16 sources.  A fold over
// constant indices, not a loop: `w` is only ever indexed by constants and stays in registers.
template <bool WIRED, uint32_t... I>
static SHA_D void sha512_fetch_all(uint64_t (&w)[16], const uint64_t* words, const uint32_t* src, const uint64_t* digests,
                                   std::integer_sequence<uint32_t, I...>) {
  if constexpr (WIRED)
    ((w[I] = sha2_load(src[I], words, digests)), ...);
  else
    ((w[I] = words[I]), ...);
}

// One lane per segment: the compression chain of one message, 80 dependent rounds per block, so the launch is
// latency-bound: one wave per workgroup spreads the segments over the CUs.  Lanes of a wave may differ in their block
// counts and their variants.  The host has checked that every lane's regions lie below n / CQ_SHA512_REGION_ROWS and its
// words inside `words`.
// Unwired (cq_sha512_synthesize_dev): lane i is segment i, its tag its variant, its message words lie at
// words + first_source, and neither `sources` nor `init_sources` is looked at.  WIRED (cq_sha512_synthesize_segments_dev):
// the launch is one level's lanes; a lane's segment sits above the variant bit of its tag, its 16 * blocks sources at
// sources + first_source and its eight initial sources (32 bytes, aligned to 16) at init_sources + 8 * segment, the
// sentinel standing for the variant's own word; `digests` is read (earlier levels') and written (this lane's segment).
template <bool WIRED>
__global__ __launch_bounds__(64) void sha512_chain_kernel(const Sha2Lane* __restrict__ lanes, uint32_t nlanes, const uint64_t* words,
                                                          uint64_t* digests, Sha512Region* __restrict__ regions,
                                                          const uint32_t* __restrict__ sources, const uint32_t* __restrict__ init_sources) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nlanes) return;
  const Sha2Lane lane = lanes[i];
  const uint32_t segment = WIRED ? lane.tag >> 1 : i;
  const uint64_t* iv = SHA512_IV_DEV[lane.tag & 1u];
  uint64_t h[8] = {iv[0], iv[1], iv[2], iv[3], iv[4], iv[5], iv[6], iv[7]};
  if constexpr (WIRED) sha2_fetch_init_all(h, init_sources + 8 * (size_t)segment, words, digests);
  Sha512Region* out = regions + lane.first_region;
  const uint64_t* msg = WIRED ? words : words + lane.first_source;
  const uint32_t* src = WIRED ? sources + lane.first_source : nullptr;
  for (uint32_t b = 0; b < lane.blocks; b++, out += CQ_SHA512_BLOCK_REGIONS)
    sha2_block(h, out, b ? SHA_RG_CHAIN : 0, [&](uint64_t (&w)[16]) {
      sha512_fetch_all<WIRED>(w, msg, src, digests, std::make_integer_sequence<uint32_t, 16>{});
      if (WIRED) src += 16; else msg += 16;
    });
  sha2_finish(h, out, digests + 8 * (size_t)segment);
}

// One thread per XOR unit of one level (cq_sha512_synthesize_xors_dev), before the level's chains on the same stream: both
// operands through sha2_load (the digests they may read are earlier levels'), the 64-bit result word behind the segments'
// digests, and the unit's two regions: e = x alone, then e = y with W = x ^ y under SHA_RG_F3, whose CHP_EVEN word the
// expansion computes as this region's e xor the one before.  `digests` is read and written, hence neither const nor
// restrict.  The host has checked every operand against both arrays' lengths and that region + 1 lies below
// n / CQ_SHA512_REGION_ROWS.
__global__ __launch_bounds__(64) void sha512_xor_kernel(const Sha2XorUnit* __restrict__ units, uint32_t nunits, const uint64_t* words,
                                                        uint64_t* digests, Sha512Region* __restrict__ regions) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nunits) return;
  const uint4 u = *reinterpret_cast<const uint4*>(units + i);
  const uint64_t x = sha2_load(u.x, words, digests), y = sha2_load(u.y, words, digests);
  digests[u.z] = x ^ y;
  sha2_put<uint64_t>(regions + u.w, 0, x, 0, 0);
  sha2_put<uint64_t>(regions + u.w + 1, 0, y, x ^ y, SHA_RG_F3);
}

// Validates the description, then queues the upload of the lanes and the message words, the chain launch, the expansion
// and the digests' download on the context's stream, and waits for the stream once.  The staging is pinned; a segment
// synthesis of sha256.hip queued before this call may still copy out of it, so its event is waited for first.
int sha512_synthesize(cq_ctx* c, uint32_t table_bits, const uint32_t* seg_blocks, size_t segments, const uint32_t* seg_variant,
                      const uint64_t* msg_words, uint32_t n, const Sha2Cols& cols, uint64_t* digests_out) {
  uint64_t regions, blocks;
  CQ_TRY(sha2_count_segments<Sha512>(c, seg_blocks, seg_variant, segments, n, regions, blocks));
  static_assert(sizeof(Sha512Region) == 32 && sizeof(Sha2Lane) == 16, "four words each");
  // lanes, then message words; the digests behind them: every part a multiple of 16 bytes
  const size_t lanes_bytes = segments * sizeof(Sha2Lane), words_bytes = 16 * blocks * sizeof(uint64_t);
  const size_t tables_bytes = lanes_bytes + words_bytes, digests_bytes = 8 * segments * sizeof(uint64_t);
  void *pin, *dev_regions, *dev_tables;
  CQ_TRY(sha2_stage(c, tables_bytes + digests_bytes, regions * sizeof(Sha512Region), tables_bytes + digests_bytes, &pin, &dev_regions, &dev_tables));
  sha2_fill_lanes<Sha512>((Sha2Lane*)pin, seg_blocks, segments, {}, {}, [&](size_t j) { return seg_variant[j]; });
  memcpy((char*)pin + lanes_bytes, msg_words, words_bytes);
  CQ_TRY(sha2_upload(c, dev_tables, pin, tables_bytes));
  const Sha2Lane* dev_lanes = (const Sha2Lane*)dev_tables;
  const uint64_t* dev_words = (const uint64_t*)((const char*)dev_tables + lanes_bytes);
  uint64_t* dev_digests = (uint64_t*)((char*)dev_tables + tables_bytes);
  sha512_chain_kernel<false><<<((uint32_t)segments + 63) / 64, 64, 0, c->stream>>>(dev_lanes, (uint32_t)segments, dev_words, dev_digests,
                                                                                  (Sha512Region*)dev_regions, nullptr, nullptr);
  if (hipGetLastError() != hipSuccess) return c->fail(CQ_ERR_HIP, "sha512_chain launch failed");
  sha512_expand_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>((const Sha512Region*)dev_regions, (uint32_t)regions, n, table_bits, cols);
  if (hipGetLastError() != hipSuccess) return c->fail(CQ_ERR_HIP, "sha512_expand launch failed");
  CQ_HIP(c, hipMemcpyAsync((char*)pin + tables_bytes, dev_digests, digests_bytes, hipMemcpyDeviceToHost, c->stream));
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  memcpy(digests_out, (const char*)pin + tables_bytes, digests_bytes);
  return CQ_OK;
}

// Validates the description, then queues the tables' upload, one chain launch per level and the expansion on the context's
// stream.  Nothing here waits for the stream: the staging is pinned, and only the previous call's copy out of it -- this
// function's, sha512_synthesize's or a segment synthesis of sha256.hip's -- is waited for, through the event they share.
// init_sources = nullptr is the description whose segments all start from their variant's initial hash value: the staged
// table then holds the sentinel everywhere, so the kernel has one form.
// n_xors = 0 is the description without XOR units: a digest reference at or above 8 * segments then names a segment that
// does not exist, and the launches and the staged bytes are those of the plain wired description.  Otherwise such a
// reference in a message word's own source names unit (index - 8 * segments) of `xors`, whose result the level's XOR
// launch stores at that word of `digests_dev` before the chains that read it run; the units ride, sorted by level, behind
// the initial sources in the same staging.
int sha512_synthesize_segments(cq_ctx* c, uint32_t table_bits, const uint32_t* seg_blocks, size_t segments, const uint32_t* seg_variant,
                               const uint32_t* sources, const uint32_t* init_sources, const uint32_t* xors, size_t n_xors,
                               const uint64_t* words_dev, size_t words_len, uint32_t n, const Sha2Cols& cols, uint64_t* digests_dev) {
  uint64_t regions, blocks;
  CQ_TRY(sha2_count_segments<Sha512>(c, seg_blocks, seg_variant, segments, n, regions, blocks));
  CQ_TRY(sha2_check_xor_units<Sha512>(c, xors, n_xors, segments, words_len, regions, n));
  std::vector<uint32_t> level(segments, 0);
  for (size_t j = 0, at = 0; j < segments; j++) {
    // a source of segment j: "" if it is good, and the segment's level follows a digest's
    auto check = [&](uint32_t s) -> std::string {
      if (s == CQ_SHA512_SOURCE_IV) return " is the initial-value sentinel, which only an initial word can be";
      return sha2_plain_source(s, j, words_len, level);
    };
    for (size_t i = 0; init_sources && i < 8; i++) {
      const uint32_t s = init_sources[8 * j + i];
      if (s == CQ_SHA512_SOURCE_IV) continue;
      const std::string bad = check(s);
      if (!bad.empty()) return c->fail(CQ_ERR_ARG, "sha512: segment " + std::to_string(j) + ", initial word " + std::to_string(i) + bad);
    }
    for (size_t t = 0; t < 16 * (size_t)seg_blocks[j]; t++, at++) {
      const uint32_t s = sources[at];
      const bool unit = s != CQ_SHA512_SOURCE_IV && sha2_reads_xor_unit(s, segments, n_xors);  // a unit's result, read like a digest word
      const std::string bad = unit ? sha2_xor_reader(s, j, segments, xors, n_xors, words_len, level) : check(s);
      if (!bad.empty()) return c->fail(CQ_ERR_ARG, "sha512: segment " + std::to_string(j) + ", word " + std::to_string(t) + bad);
    }
  }
  const Sha2Levels lv = sha2_levels(level);
  const Sha2XorLevels xl = sha2_xor_levels(xors, n_xors, level, lv.count.size());

  // lanes, sources, initial sources, xor units: each a multiple of 16 bytes, so a segment's eight initial sources and the
  // units are aligned for their 16-byte loads
  const size_t lanes_bytes = segments * sizeof(Sha2Lane), sources_bytes = 16 * blocks * sizeof(uint32_t);
  const size_t init_bytes = 8 * segments * sizeof(uint32_t), xors_bytes = n_xors * sizeof(Sha2XorUnit);
  const size_t tables_bytes = lanes_bytes + sources_bytes + init_bytes + xors_bytes;
  const uint64_t all_regions = regions + CQ_SHA512_XOR_REGIONS * (uint64_t)n_xors;  // the units' regions lie behind the last tail
  void *pin, *dev_regions, *dev_tables;
  CQ_TRY(sha2_stage(c, tables_bytes, all_regions * sizeof(Sha512Region), tables_bytes, &pin, &dev_regions, &dev_tables));
  sha2_fill_lanes<Sha512>((Sha2Lane*)pin, seg_blocks, segments, level, lv, [&](size_t j) { return (uint32_t)j << 1 | seg_variant[j]; });
  memcpy((char*)pin + lanes_bytes, sources, sources_bytes);
  uint32_t* staged_init = (uint32_t*)((char*)pin + lanes_bytes + sources_bytes);
  if (init_sources) memcpy(staged_init, init_sources, init_bytes);
  else std::fill(staged_init, staged_init + 8 * segments, CQ_SHA512_SOURCE_IV);
  sha2_fill_xor_units((Sha2XorUnit*)((char*)staged_init + init_bytes), xors, n_xors, xl, segments, regions);
  CQ_TRY(sha2_upload(c, dev_tables, pin, tables_bytes));
  const Sha2Lane* dev_lanes = (const Sha2Lane*)dev_tables;
  const uint32_t* dev_sources = (const uint32_t*)((const char*)dev_tables + lanes_bytes);
  const uint32_t* dev_init = (const uint32_t*)((const char*)dev_sources + sources_bytes);
  const Sha2XorUnit* dev_units = (const Sha2XorUnit*)((const char*)dev_init + init_bytes);
  auto launch_xors = [&](size_t l) {  // the units that are ready at level l, if there are any
    if (l >= xl.count.size() || !xl.count[l]) return true;
    sha512_xor_kernel<<<(xl.count[l] + 63) / 64, 64, 0, c->stream>>>(dev_units + xl.first[l], xl.count[l], words_dev, digests_dev,
                                                                    (Sha512Region*)dev_regions);
    return hipGetLastError() == hipSuccess;
  };
  for (size_t l = 0; l < lv.count.size(); l++) {
    if (!launch_xors(l)) return c->fail(CQ_ERR_HIP, "sha512_xor launch failed");
    sha512_chain_kernel<true><<<(lv.count[l] + 63) / 64, 64, 0, c->stream>>>(dev_lanes + lv.first[l], lv.count[l], words_dev, digests_dev,
                                                                            (Sha512Region*)dev_regions, dev_sources, dev_init);
    if (hipGetLastError() != hipSuccess) return c->fail(CQ_ERR_HIP, "sha512_chain launch failed");
  }
  if (!launch_xors(lv.count.size())) return c->fail(CQ_ERR_HIP, "sha512_xor launch failed");  // units over the last level's digests
  sha512_expand_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>((const Sha512Region*)dev_regions, (uint32_t)all_regions, n, table_bits, cols);
  if (hipGetLastError() != hipSuccess) return c->fail(CQ_ERR_HIP, "sha512_expand launch failed");
  return CQ_OK;
}

}  // namespace cq

using namespace cq;

extern "C" {

int cq_sha512_layout(uint32_t* cells, size_t cap, size_t* count) {
  if (!count || (cap && !cells)) return CQ_ERR_ARG;
  *count = SHA512_NUM_CELLS;
  for (size_t i = 0; i < cap && i < SHA512_NUM_CELLS; i++) {
    const Sha256Cell& s = SHA512_CELLS[i];
    const uint32_t words[CQ_SHA256_CELL_WORDS] = {s.kind, s.form, s.column, s.row, s.offset, s.per_table_bits, s.len};
    for (uint32_t j = 0; j < CQ_SHA256_CELL_WORDS; j++) cells[i * CQ_SHA256_CELL_WORDS + j] = words[j];
  }
  return CQ_OK;
}

int cq_sha512_synthesize_dev(cq_ctx* c, uint32_t table_bits, const uint32_t* seg_blocks, size_t segments, const uint32_t* seg_variant,
                             const uint64_t* msg_words, size_t n, uint64_t* const* cols_dev, uint64_t* digests_out) {
  if (!c) return CQ_ERR_ARG;
  const bool bad = !seg_blocks || !seg_variant || !msg_words || !cols_dev || !digests_out || segments == 0 || n > 0x7fffffffull || segments > n;
  Sha2Cols sc;
  CQ_TRY(sha2_entry(c, "sha512", bad ? SHA2_BAD_ARGS : nullptr, table_bits, CQ_SHA512_MIN_TABLE_BITS, CQ_SHA512_MAX_TABLE_BITS, "the pieces", cols_dev, sc));
  return sha512_synthesize(c, table_bits, seg_blocks, segments, seg_variant, msg_words, (uint32_t)n, sc, digests_out);
}

// both entry points below: the argument checks that need no description, then the host function
static int sha512_segments_entry(cq_ctx* c, uint32_t table_bits, const uint32_t* seg_blocks, size_t segments, const uint32_t* seg_variant,
                                 const uint32_t* sources, const uint32_t* init_sources, const uint32_t* xors, size_t n_xors,
                                 const uint64_t* words_dev, size_t words_len, size_t n, uint64_t* const* cols_dev, uint64_t* digests_dev) {
  if (!c) return CQ_ERR_ARG;
  const char* bad = nullptr;
  if (!seg_blocks || !seg_variant || !sources || !cols_dev || !digests_dev || segments == 0 || n > 0x7fffffffull || segments > n ||
      (!words_dev && words_len) || words_len > CQ_SHA512_SOURCE_DIGEST)
    bad = SHA2_BAD_ARGS;
  else if (n_xors && (!xors || n_xors > n))
    bad = "null xor table, or more xor units than rows";
  Sha2Cols sc;
  CQ_TRY(sha2_entry(c, "sha512", bad, table_bits, CQ_SHA512_MIN_TABLE_BITS, CQ_SHA512_MAX_TABLE_BITS, "the pieces", cols_dev, sc));
  return sha512_synthesize_segments(c, table_bits, seg_blocks, segments, seg_variant, sources, init_sources, xors, n_xors, words_dev, words_len,
                                    (uint32_t)n, sc, digests_dev);
}

int cq_sha512_synthesize_segments_dev(cq_ctx* c, uint32_t table_bits, const uint32_t* seg_blocks, size_t segments, const uint32_t* seg_variant,
                                      const uint32_t* sources, const uint32_t* init_sources, const uint64_t* words_dev, size_t words_len, size_t n,
                                      uint64_t* const* cols_dev, uint64_t* digests_dev) {
  return sha512_segments_entry(c, table_bits, seg_blocks, segments, seg_variant, sources, init_sources, nullptr, 0, words_dev, words_len, n, cols_dev,
                               digests_dev);
}

int cq_sha512_synthesize_xors_dev(cq_ctx* c, uint32_t table_bits, const uint32_t* seg_blocks, size_t segments, const uint32_t* seg_variant,
                                  const uint32_t* sources, const uint32_t* init_sources, const uint32_t* xors, size_t n_xors,
                                  const uint64_t* words_dev, size_t words_len, size_t n, uint64_t* const* cols_dev, uint64_t* digests_dev) {
  return sha512_segments_entry(c, table_bits, seg_blocks, segments, seg_variant, sources, init_sources, xors, n_xors, words_dev, words_len, n, cols_dev,
                               digests_dev);
}

}  // extern "C"

// What the SHA-256 and the SHA-512 witness syntheses share, written once over a family record per word width: the bit
// functions, the words of a region the expansion kernels place, the compression chain the chain kernels run, and the host
// side's description checks, level order, the checks and levels of XOR units, pinned staging and entry preamble.
// sha256.hip and sha512.hip keep what differs: the kernels themselves (names, template parameters and launch shapes are
// theirs), how a cell's value is placed and encoded (one 64-bit limb or two), the round constants' storage, the 32-bit
// host chain, choices and variable length.
#pragma once
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "cq.hpp"
#include "ctx.hpp"
#include "sha256_layout.hpp"

namespace cq {

// region kinds (Sha2Region::meta, low byte; the round number sits above it)
constexpr uint32_t SHA_RG_ROUND = 1;  // a compression round: the additions that give a_r and e_r, the copy of K_r
constexpr uint32_t SHA_RG_SCHED = 2;  // rounds 16 and up: W_r is a schedule word
constexpr uint32_t SHA_RG_CHAIN = 4;  // incoming state of a block after the first, or the final state: H + (a .. h)
constexpr uint32_t SHA_RG_F3 = 8;     // Maj and Ch are laid out (the two regions before this one hold state words)

template <typename Word>
struct Sha2Region {
  Word a, e, w, meta;
};

// One chain of a launch: where its regions and its 16 * blocks message words (or their sources) start, and what the
// kernel needs to know of its segment -- the 32-bit kernels its index, the 64-bit ones its variant, under the index if wired.
struct Sha2Lane {
  uint32_t first_region, blocks, first_source, tag;
};

struct Sha2Cols {
  Fr* p[CQ_SHA256_ADVICE_COLUMNS];
};

// The family record of a word width.  S0 / S1: the rotations of Sigma0 / Sigma1; G0 / G1: the two rotations and the shift
// of sigma0 / sigma1.  k(t): round constant t, from the translation unit's own __constant__ table.
template <typename W>
struct Sha2Family;
template <>
struct Sha2Family<uint32_t> {
  using Word = uint32_t;
  using Region = Sha2Region<Word>;
  static constexpr const char* NAME = "sha256";
  static constexpr uint32_t ROUNDS = 64, REGION_ROWS = CQ_SHA256_REGION_ROWS, BLOCK_REGIONS = CQ_SHA256_BLOCK_REGIONS, TAIL_REGIONS = CQ_SHA256_TAIL_REGIONS;
  static constexpr uint32_t S0a = 2, S0b = 13, S0c = 22, S1a = 6, S1b = 11, S1c = 25, G0a = 7, G0b = 18, G0s = 3, G1a = 17, G1b = 19, G1s = 10;
  static __device__ __forceinline__ Word k(uint32_t t);
};
template <>
struct Sha2Family<uint64_t> {
  using Word = uint64_t;
  using Region = Sha2Region<Word>;
  static constexpr const char* NAME = "sha512";
  static constexpr uint32_t ROUNDS = 80, REGION_ROWS = CQ_SHA512_REGION_ROWS, BLOCK_REGIONS = CQ_SHA512_BLOCK_REGIONS, TAIL_REGIONS = CQ_SHA512_TAIL_REGIONS;
  static constexpr uint32_t S0a = 28, S0b = 34, S0c = 39, S1a = 14, S1b = 18, S1c = 41, G0a = 1, G0b = 8, G0s = 7, G1a = 19, G1b = 61, G1s = 6;
  static __device__ __forceinline__ Word k(uint32_t t);
};
static_assert(CQ_SHA512_SOURCE_DIGEST == CQ_SHA256_SOURCE_DIGEST && CQ_SHA512_SOURCE_IV == CQ_SHA256_SOURCE_IV, "one encoding of a source");

#define SHA_HD __host__ __device__ __forceinline__
#define SHA_D __device__ __forceinline__
template <typename W> static SHA_HD W rotr(W x, uint32_t n) { return (x >> n) | (x << (8 * sizeof(W) - n)); }  // 0 < n < the width at every use
template <typename W> static SHA_HD W xor3(W x, W y, W z) { return x ^ y ^ z; }
template <typename W> static SHA_HD W maj3(W x, W y, W z) { return (x & y) | (x & z) | (y & z); }
template <typename W> static SHA_HD W ch3(W e, W f, W g) { return (e & f) | (~e & g); }
template <typename W> static SHA_HD W big_sigma0(W a) { using F = Sha2Family<W>; return xor3(rotr(a, F::S0a), rotr(a, F::S0b), rotr(a, F::S0c)); }
template <typename W> static SHA_HD W big_sigma1(W e) { using F = Sha2Family<W>; return xor3(rotr(e, F::S1a), rotr(e, F::S1b), rotr(e, F::S1c)); }
template <typename W> static SHA_HD W small_sigma0(W w) { using F = Sha2Family<W>; return xor3(rotr(w, F::G0a), rotr(w, F::G0b), W(w >> F::G0s)); }
template <typename W> static SHA_HD W small_sigma1(W w) { using F = Sha2Family<W>; return xor3(rotr(w, F::G1a), rotr(w, F::G1b), W(w >> F::G1s)); }

// bit i -> bit 2i of a 32-bit word
static SHA_D uint64_t spread32(uint32_t w) {
  uint64_t x = w;
  x = (x | (x << 16)) & 0x0000ffff0000ffffull;
  x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
  x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
  x = (x | (x << 2)) & 0x3333333333333333ull;
  x = (x | (x << 1)) & 0x5555555555555555ull;
  return x;
}

// The carries out of the word of x + rest..., summed left to right: a 32-bit sum is taken in 64 bits, a 64-bit sum counts
// the carry of every addition.  Two sums that start with the same terms share them.
template <typename... W>
static SHA_D uint32_t sum_carry(uint32_t x, W... rest) {
  return (uint32_t)(((uint64_t)x + ... + (uint64_t)rest) >> 32);
}
template <typename... W>
static SHA_D uint32_t sum_carry(uint64_t x, W... rest) {
  uint32_t carry = 0;
  ((x += rest, carry += x < rest ? 1u : 0u), ...);
  return carry;
}

// The words of region g that the layout's cells are fields of: A, E, W and the eight even / odd words of the sigmas, then
// what the region's kind adds from its neighbours.  Every index into `regions` is guarded by the kind the chain sets and by
// the region index itself; `src` is only ever indexed by constants and stays in registers.
template <typename W>
static SHA_D void sha2_fill_src(W (&src)[CQ_SHA256_SRC_COUNT], const Sha2Region<W>* __restrict__ regions, uint32_t g) {
  using F = Sha2Family<W>;
  const Sha2Region<W> cur = regions[g];
  const uint32_t kind = (uint32_t)cur.meta & 0xffu;
  CQ_UNROLL for (uint32_t i = 0; i < CQ_SHA256_SRC_COUNT; i++) src[i] = 0;
  src[CQ_SHA256_SRC_A] = cur.a;
  src[CQ_SHA256_SRC_E] = cur.e;
  src[CQ_SHA256_SRC_W] = cur.w;
  src[CQ_SHA256_SRC_S0_EVEN] = big_sigma0(cur.a);
  src[CQ_SHA256_SRC_S0_ODD] = maj3(rotr(cur.a, F::S0a), rotr(cur.a, F::S0b), rotr(cur.a, F::S0c));
  src[CQ_SHA256_SRC_S1_EVEN] = big_sigma1(cur.e);
  src[CQ_SHA256_SRC_S1_ODD] = maj3(rotr(cur.e, F::S1a), rotr(cur.e, F::S1b), rotr(cur.e, F::S1c));
  src[CQ_SHA256_SRC_G0_EVEN] = small_sigma0(cur.w);
  src[CQ_SHA256_SRC_G0_ODD] = maj3(rotr(cur.w, F::G0a), rotr(cur.w, F::G0b), W(cur.w >> F::G0s));
  src[CQ_SHA256_SRC_G1_EVEN] = small_sigma1(cur.w);
  src[CQ_SHA256_SRC_G1_ODD] = maj3(rotr(cur.w, F::G1a), rotr(cur.w, F::G1b), W(cur.w >> F::G1s));
  if ((kind & SHA_RG_F3) && g >= 2) {
    const Sha2Region<W> p1 = regions[g - 1], p2 = regions[g - 2];
    src[CQ_SHA256_SRC_MAJ_EVEN] = xor3(cur.a, p1.a, p2.a);
    src[CQ_SHA256_SRC_MAJ_ODD] = maj3(cur.a, p1.a, p2.a);
    src[CQ_SHA256_SRC_CHP_EVEN] = cur.e ^ p1.e;
    src[CQ_SHA256_SRC_CHP_ODD] = cur.e & p1.e;
    src[CQ_SHA256_SRC_CHQ_EVEN] = ~cur.e ^ p2.e;
    src[CQ_SHA256_SRC_CHQ_ODD] = ~cur.e & p2.e;
    src[CQ_SHA256_SRC_CH] = ch3(cur.e, p1.e, p2.e);
  }
  if ((kind & SHA_RG_ROUND) && g >= 4) {  // T1 = h + Sigma1(e) + Ch(e, f, g) + K + W; e_r = T1 + d; a_r = T1 + Sigma0(a) + Maj(a, b, c)
    const Sha2Region<W> p1 = regions[g - 1], p2 = regions[g - 2], p3 = regions[g - 3], p4 = regions[g - 4];
    const W k = F::k(((uint32_t)cur.meta >> 8) % F::ROUNDS), s1 = big_sigma1(p1.e), ch = ch3(p1.e, p2.e, p3.e);
    src[CQ_SHA256_SRC_K] = k;
    src[CQ_SHA256_SRC_CARRY_E] = sum_carry(p4.e, s1, ch, k, cur.w, p4.a);
    src[CQ_SHA256_SRC_CARRY_A] = sum_carry(p4.e, s1, ch, k, cur.w, big_sigma0(p1.a), maj3(p1.a, p2.a, p3.a));
  }
  if ((kind & SHA_RG_SCHED) && g >= 16)
    src[CQ_SHA256_SRC_CARRY_W] = sum_carry(small_sigma1(regions[g - 2].w), regions[g - 7].w, small_sigma0(regions[g - 15].w), regions[g - 16].w);
  if ((kind & SHA_RG_CHAIN) && g >= F::BLOCK_REGIONS) {
    const Sha2Region<W> h = regions[g - F::BLOCK_REGIONS], v = regions[g - 4];
    src[CQ_SHA256_SRC_CARRY_A] = sum_carry(h.a, v.a);
    src[CQ_SHA256_SRC_CARRY_E] = sum_carry(h.e, v.e);
  }
}

// ---- the compression chain on the device -------------------------------------------------------------------------------

template <typename W>
static SHA_D void sha2_put(Sha2Region<W>* p, W a, W e, W w, uint32_t meta) {
  if constexpr (sizeof(W) == 4) {
    *reinterpret_cast<uint4*>(p) = make_uint4(a, e, w, meta);
  } else {
    ulonglong2* q = reinterpret_cast<ulonglong2*>(p);
    q[0] = make_ulonglong2(a, e);
    q[1] = make_ulonglong2(w, meta);
  }
}

// a_-4 .. a_-1 = d, c, b, a and e_-4 .. e_-1 = h, g, f, e
template <typename W>
static SHA_D void sha2_put_state(Sha2Region<W>* out, const W (&h)[8], uint32_t chain) {
  sha2_put<W>(out + 0, h[3], h[7], 0, chain);
  sha2_put<W>(out + 1, h[2], h[6], 0, chain);
  sha2_put<W>(out + 2, h[1], h[5], 0, chain | SHA_RG_F3);
  sha2_put<W>(out + 3, h[0], h[4], 0, chain | SHA_RG_F3);
}

// Round T0 + I on the 16-word rolling schedule and the state (a .. h), and its region.  I is a compile-time constant, so
// `w` and `s` are only ever indexed by constants and stay in registers; T0, the group's first round, may be a loop variable.
template <bool SCHED, uint32_t I, typename W>
static SHA_D void sha2_step(W (&s)[8], W (&w)[16], uint32_t t0, Sha2Region<W>* out) {
  if (SCHED) w[I] += small_sigma1(w[(I + 14) & 15]) + w[(I + 9) & 15] + small_sigma0(w[(I + 1) & 15]);
  const W t1 = s[7] + big_sigma1(s[4]) + ch3(s[4], s[5], s[6]) + Sha2Family<W>::k(t0 + I) + w[I];
  const W t2 = big_sigma0(s[0]) + maj3(s[0], s[1], s[2]);
  s[7] = s[6], s[6] = s[5], s[5] = s[4], s[4] = s[3] + t1;
  s[3] = s[2], s[2] = s[1], s[1] = s[0], s[0] = t1 + t2;
  sha2_put<W>(out + t0 + I, s[0], s[4], w[I], SHA_RG_ROUND | SHA_RG_F3 | (SCHED ? SHA_RG_SCHED : 0) | (t0 + I) << 8);
}
template <bool SCHED, typename W, uint32_t... I>
static SHA_D void sha2_steps(W (&s)[8], W (&w)[16], uint32_t t0, Sha2Region<W>* out, std::integer_sequence<uint32_t, I...>) {
  (sha2_step<SCHED, I>(s, w, t0, out), ...);
}

// A plain source: a word of the caller's buffer or a digest word an earlier level's launch stored.  The host has checked
// every source against both arrays' lengths.
template <typename W>
static SHA_D W sha2_load(uint32_t s, const W* words, const W* digests) {
  return *((s & CQ_SHA256_SOURCE_DIGEST) ? digests + (s & (CQ_SHA256_SOURCE_DIGEST - 1)) : words + s);
}

// Word I of the state a lane's chain starts from: the one `h` holds already on the sentinel, else a plain source read from
// `init_words` / `digests`.  I is a compile-time constant, so `h` stays in registers.
template <uint32_t I, typename W>
static SHA_D void sha2_fetch_init(W (&h)[8], uint32_t s, const W* init_words, const W* digests) {
  if (s != CQ_SHA256_SOURCE_IV) h[I] = sha2_load(s, init_words, digests);
}
// the eight of a segment: 32 bytes at `sources`, aligned to 16
template <typename W>
static SHA_D void sha2_fetch_init_all(W (&h)[8], const uint32_t* sources, const W* init_words, const W* digests) {
  const uint4* is = reinterpret_cast<const uint4*>(sources);
  const uint4 lo = is[0], hi = is[1];
  sha2_fetch_init<0>(h, lo.x, init_words, digests), sha2_fetch_init<1>(h, lo.y, init_words, digests);
  sha2_fetch_init<2>(h, lo.z, init_words, digests), sha2_fetch_init<3>(h, lo.w, init_words, digests);
  sha2_fetch_init<4>(h, hi.x, init_words, digests), sha2_fetch_init<5>(h, hi.y, init_words, digests);
  sha2_fetch_init<6>(h, hi.z, init_words, digests), sha2_fetch_init<7>(h, hi.w, init_words, digests);
}

// One block of a chain: the state regions in front of it, the 16 message words `fetch(w)` gives, the rounds and their
// regions, and H += (a .. h).  `chain`: SHA_RG_CHAIN for a block after the first.
template <typename W, typename Fetch>
static SHA_D void sha2_block(W (&h)[8], Sha2Region<W>* out, uint32_t chain, Fetch fetch) {
  using Seq16 = std::make_integer_sequence<uint32_t, 16>;
  sha2_put_state(out, h, chain);
  W w[16], s[8] = {h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7]};
  fetch(w);
  sha2_steps<false>(s, w, 0, out + 4, Seq16{});
  for (uint32_t t0 = 16; t0 < Sha2Family<W>::ROUNDS; t0 += 16) sha2_steps<true>(s, w, t0, out + 4, Seq16{});
  h[0] += s[0], h[1] += s[1], h[2] += s[2], h[3] += s[3];
  h[4] += s[4], h[5] += s[5], h[6] += s[6], h[7] += s[7];
}

// behind a lane's last block: the final state's regions, and its eight words for later levels and the caller
template <typename W>
static SHA_D void sha2_finish(const W (&h)[8], Sha2Region<W>* out, W* d) {
  sha2_put_state(out, h, SHA_RG_CHAIN);
  d[0] = h[0], d[1] = h[1], d[2] = h[2], d[3] = h[3], d[4] = h[4], d[5] = h[5], d[6] = h[6], d[7] = h[7];
}

// ---- host side ----------------------------------------------------------------------------------------------------------

// Every segment has a block -- and, where the family has variants, one of them -- and the segments up to each fit the
// rows; `more(j)` is the caller's own check of segment j behind these.  Leaves the sums of the regions and the blocks.
template <typename F, typename More>
static int sha2_count_segments(cq_ctx* c, const uint32_t* seg_blocks, const uint32_t* seg_variant, size_t segments, uint32_t n, uint64_t& regions,
                               uint64_t& blocks, More more) {
  const std::string name = F::NAME;
  const uint64_t max_regions = n / F::REGION_ROWS;
  regions = blocks = 0;
  for (size_t j = 0; j < segments; j++) {
    if (seg_blocks[j] == 0) return c->fail(CQ_ERR_ARG, name + ": segment " + std::to_string(j) + " has no block");
    if (seg_variant && seg_variant[j] != CQ_SHA512_VARIANT_512 && seg_variant[j] != CQ_SHA512_VARIANT_384)
      return c->fail(CQ_ERR_ARG, name + ": segment " + std::to_string(j) + " has variant " + std::to_string(seg_variant[j]));
    blocks += seg_blocks[j];
    regions += (uint64_t)seg_blocks[j] * F::BLOCK_REGIONS + F::TAIL_REGIONS;
    if (regions > max_regions) return c->fail(CQ_ERR_ARG, name + ": the segments up to segment " + std::to_string(j) + " do not fit the rows");
    CQ_TRY(more(j));
  }
  return CQ_OK;
}
template <typename F>
static int sha2_count_segments(cq_ctx* c, const uint32_t* seg_blocks, const uint32_t* seg_variant, size_t segments, uint32_t n, uint64_t& regions,
                               uint64_t& blocks) {
  return sha2_count_segments<F>(c, seg_blocks, seg_variant, segments, n, regions, blocks, [](size_t) { return CQ_OK; });
}

// A plain source of segment j -- a message word's, an initial word's or an operand's: "" if it is good, else what is wrong
// with it; the segment's level follows that of a digest it reads.
static inline std::string sha2_plain_source(uint32_t s, size_t j, size_t words_len, std::vector<uint32_t>& level) {
  if (s & CQ_SHA256_SOURCE_DIGEST) {
    const size_t ref = (s & (CQ_SHA256_SOURCE_DIGEST - 1)) >> 3;
    if (ref >= j) return " reads the digest of segment " + std::to_string(ref) + ", which does not come before it";
    if (level[ref] + 1 > level[j]) level[j] = level[ref] + 1;
  } else if (s >= words_len) {
    return " reads word " + std::to_string(s) + " of a buffer of " + std::to_string(words_len);
  }
  return "";
}

// How many segments each level has, and where a level's lanes start when the lanes stand in level order.
struct Sha2Levels {
  std::vector<uint32_t> count, first;
};
static inline Sha2Levels sha2_levels(const std::vector<uint32_t>& level) {
  Sha2Levels lv;
  for (uint32_t l : level) {
    if (l >= lv.count.size()) lv.count.resize(l + 1, 0);
    lv.count[l]++;
  }
  lv.first.assign(lv.count.size(), 0);
  for (size_t l = 1; l < lv.count.size(); l++) lv.first[l] = lv.first[l - 1] + lv.count[l - 1];
  return lv;
}

// ---- XOR units: a message word that is the XOR of two plain sources ----------------------------------------------------

// One XOR unit as the device sees it at both widths: its two operands (plain sources), the word of `digests` that takes
// the result, and -- both filled in by the host -- the first of the unit's two regions.
struct Sha2XorUnit {
  uint32_t x, y, result, region;
};
static_assert(CQ_SHA512_XOR_WORDS == CQ_SHA256_XOR_WORDS && CQ_SHA512_XOR_REGIONS == CQ_SHA256_XOR_REGIONS, "one table of units, one area");
static_assert(sizeof(Sha2XorUnit) == CQ_SHA256_XOR_WORDS * sizeof(uint32_t), "an entry of the xor table as the header states it");

// The units' area behind `regions` regions of segments fits n rows, and every operand is a plain source: a word of the
// buffer or a digest word of a segment that exists (no unit's result).
template <typename F>
static int sha2_check_xor_units(cq_ctx* c, const uint32_t* xors, size_t n_xors, size_t segments, size_t words_len, uint64_t regions, uint32_t n) {
  const std::string name = F::NAME;
  if (regions + CQ_SHA256_XOR_REGIONS * (uint64_t)n_xors > n / F::REGION_ROWS)
    return c->fail(CQ_ERR_ARG, name + ": the area of " + std::to_string(n_xors) + " xor units behind the segments does not fit the rows");
  for (size_t u = 0; u < n_xors; u++)
    for (uint32_t o = 0; o < 2; o++) {
      const uint32_t s = xors[CQ_SHA256_XOR_WORDS * u + o];
      std::string bad;
      if (s & CQ_SHA256_SOURCE_DIGEST) {
        const size_t ref = (s & (CQ_SHA256_SOURCE_DIGEST - 1)) >> 3;
        if (ref >= segments) bad = " reads the digest of segment " + std::to_string(ref) + " of " + std::to_string(segments);
      } else if (s >= words_len) {
        bad = " reads word " + std::to_string(s) + " of a buffer of " + std::to_string(words_len);
      }
      if (!bad.empty()) return c->fail(CQ_ERR_ARG, name + ": xor unit " + std::to_string(u) + (o ? ", operand y" : ", operand x") + bad);
    }
  return CQ_OK;
}

// whether a message word's source names a unit's result: a digest reference behind the segments' own words
static inline bool sha2_reads_xor_unit(uint32_t s, size_t segments, size_t n_xors) {
  return n_xors && (s & CQ_SHA256_SOURCE_DIGEST) && (s & (CQ_SHA256_SOURCE_DIGEST - 1)) >= 8 * segments;
}

// Such a source of a word of segment j: "" if it is good, else what is wrong with it.  The unit's digest operands come
// before the segment, and the segment runs at or above the unit's level.
static inline std::string sha2_xor_reader(uint32_t s, size_t j, size_t segments, const uint32_t* xors, size_t n_xors, size_t words_len,
                                          std::vector<uint32_t>& level) {
  const size_t u = (s & (CQ_SHA256_SOURCE_DIGEST - 1)) - 8 * segments;
  if (u >= n_xors) return " reads xor unit " + std::to_string(u) + " of " + std::to_string(n_xors);
  for (uint32_t o = 0; o < 2; o++) {
    const std::string bad = sha2_plain_source(xors[CQ_SHA256_XOR_WORDS * u + o], j, words_len, level);
    if (!bad.empty()) return ", xor unit " + std::to_string(u) + (o ? ", operand y" : ", operand x") + bad;
  }
  return "";
}

// A unit is ready at level 0 if it reads no digest, else one level above the highest level it reads: at most one level
// behind the last chain launch.  `level`: every segment's, final, whether or not a word reads the unit.  `count` and
// `first` are per level, as Sha2Levels', with one level more than the chains have; all three are empty without units.
struct Sha2XorLevels {
  std::vector<uint32_t> level, count, first;
};
static inline Sha2XorLevels sha2_xor_levels(const uint32_t* xors, size_t n_xors, const std::vector<uint32_t>& level, size_t chain_levels) {
  Sha2XorLevels xl;
  xl.level.assign(n_xors, 0);
  xl.count.assign(n_xors ? chain_levels + 1 : 0, 0);
  for (size_t u = 0; u < n_xors; u++) {
    for (uint32_t o = 0; o < 2; o++) {
      const uint32_t s = xors[CQ_SHA256_XOR_WORDS * u + o];
      if (s & CQ_SHA256_SOURCE_DIGEST) xl.level[u] = std::max(xl.level[u], level[(s & (CQ_SHA256_SOURCE_DIGEST - 1)) >> 3] + 1);
    }
    xl.count[xl.level[u]]++;
  }
  xl.first.assign(xl.count.size(), 0);
  for (size_t l = 1; l < xl.count.size(); l++) xl.first[l] = xl.first[l - 1] + xl.count[l - 1];
  return xl;
}

// The units in level order; unit u keeps its result word, 8 * segments + u, and its regions, behind the segments' `regions`,
// whatever its level.
static inline void sha2_fill_xor_units(Sha2XorUnit* units, const uint32_t* xors, size_t n_xors, const Sha2XorLevels& xl, size_t segments,
                                       uint64_t regions) {
  std::vector<uint32_t> next = xl.first;
  for (size_t u = 0; u < n_xors; u++)
    units[next[xl.level[u]]++] = {xors[CQ_SHA256_XOR_WORDS * u], xors[CQ_SHA256_XOR_WORDS * u + 1], (uint32_t)(8 * segments + u),
                                  (uint32_t)(regions + CQ_SHA256_XOR_REGIONS * u)};
}

// The lanes in level order, segments of one level in row order; `tag(j)` is Sha2Lane::tag of segment j.  One level (an
// empty `level`) leaves lane j = segment j.
template <typename F, typename Tag>
static void sha2_fill_lanes(Sha2Lane* lanes, const uint32_t* seg_blocks, size_t segments, const std::vector<uint32_t>& level, const Sha2Levels& lv,
                            Tag tag) {
  std::vector<uint32_t> next = level.empty() ? std::vector<uint32_t>(1, 0) : lv.first;
  uint32_t first_region = 0, first_source = 0;
  for (size_t j = 0; j < segments; j++) {
    lanes[next[level.empty() ? 0 : level[j]]++] = {first_region, seg_blocks[j], first_source, tag(j)};
    first_region += seg_blocks[j] * F::BLOCK_REGIONS + F::TAIL_REGIONS;
    first_source += 16 * seg_blocks[j];
  }
}

// The pinned staging of a call's tables, shared by every synthesis of both widths.  sha2_stage waits for the previous
// call's copy out of the staging (at once if there was none), then makes sure of the staging and of both scratch buffers;
// sha2_upload queues the copy of the filled staging and records the event the next call waits for.  The wait comes before
// the buffers may move: cq_ctx::grow synchronises the stream before it frees, so waiting behind it would do as well, but
// this order needs no such argument.
static inline int sha2_stage(cq_ctx* c, size_t pinned_bytes, size_t regions_bytes, size_t tables_bytes, void** pin, void** dev_regions,
                             void** dev_tables) {
  if (c->sha_staged) CQ_HIP(c, hipEventSynchronize(c->sha_staged));
  else CQ_HIP(c, hipEventCreateWithFlags(&c->sha_staged, hipEventDisableTiming));
  CQ_TRY(c->ensure_pinned_sha(pinned_bytes, pin));
  CQ_TRY(c->ensure_scratch(Scratch::EntryA, regions_bytes, dev_regions));
  return c->ensure_scratch(Scratch::EntryB, tables_bytes, dev_tables);
}
static inline int sha2_upload(cq_ctx* c, void* dev_tables, const void* pin, size_t bytes) {
  CQ_HIP(c, hipMemcpyAsync(dev_tables, pin, bytes, hipMemcpyHostToDevice, c->stream));
  CQ_HIP(c, hipEventRecord(c->sha_staged, c->stream));
  return CQ_OK;
}

// What every entry point does before its host function.  `bad`: what the entry's own look at its arguments found (nullptr:
// nothing), SHA2_BAD_ARGS for the checks every entry has; then the table_bits range -- `fit`: what has to fit it -- the
// device, and the 18 column pointers.
constexpr const char* SHA2_BAD_ARGS = "null array, no segment, or a length out of range";
static inline int sha2_entry(cq_ctx* c, const char* name, const char* bad, uint32_t table_bits, uint32_t min_bits, uint32_t max_bits, const char* fit,
                             uint64_t* const* cols_dev, Sha2Cols& sc) {
  const std::string prefix = std::string(name) + ": ";
  if (bad) return c->fail(CQ_ERR_ARG, prefix + bad);
  if (table_bits < min_bits || table_bits > max_bits) return c->fail(CQ_ERR_ARG, prefix + "table_bits outside the range " + fit + " fit");
  CQ_HIP(c, hipSetDevice(c->device));
  for (uint32_t i = 0; i < CQ_SHA256_ADVICE_COLUMNS; i++) {
    if (!cols_dev[i]) return c->fail(CQ_ERR_ARG, prefix + "null column");
    sc.p[i] = (Fr*)cols_dev[i];
  }
  return CQ_OK;
}

}  // namespace cq

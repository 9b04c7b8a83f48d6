// SHA-512 / SHA-384 compression circuit: witness synthesis.  The 64-bit counterpart of sha256.hip's segment path without
// wiring: every segment is an independent message, so one launch runs all the compression chains, one lane per segment
// (80 sequential rounds per 128-byte block), and leaves four 64-bit words per region on the device -- a_r, e_r, W_r and
// what kind of region it is.  The expansion kernel turns them into the 18 advice columns, one thread per row: every cell
// is a bit field of a word that a handful of xors and additions of the region's and its neighbours' (a, e, W) give,
// placed by the layout table of sha512_layout.hpp.  The spread form of a 64-bit word has 128 bits, so a cell value is two
// 64-bit limbs until it is Montgomery-encoded.
#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "cq.hpp"
#include "ctx.hpp"
#include "sha512_layout.hpp"
#include "tablehash.hpp"

namespace cq {

// region kinds (Sha512Region::meta, low byte; the round number sits above it): sha256.hip's, with 80 rounds
constexpr uint32_t SHA512_RG_ROUND = 1;  // a compression round: the additions that give a_r and e_r, the copy of K_r
constexpr uint32_t SHA512_RG_SCHED = 2;  // rounds 16 .. 79: W_r is a schedule word
constexpr uint32_t SHA512_RG_CHAIN = 4;  // incoming state of a block after the first, or the final state: H + (a .. h)
constexpr uint32_t SHA512_RG_F3 = 8;     // Maj and Ch are laid out (the two regions before this one hold state words)

struct Sha512Region {
  uint64_t a, e, w, meta;
};

// One chain: where its regions and its 16 * blocks message words start, and which initial hash value it starts from.
struct Sha512Lane {
  uint32_t first_region, blocks, first_word, variant;
};

struct Sha512Cols {
  Fr* p[CQ_SHA256_ADVICE_COLUMNS];
};

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

#define SHA_D __device__ __forceinline__
static SHA_D uint64_t rotr64(uint64_t x, uint32_t n) { return (x >> n) | (x << (64 - n)); }  // 0 < n < 64 at every use
static SHA_D uint64_t xor3(uint64_t x, uint64_t y, uint64_t z) { return x ^ y ^ z; }
static SHA_D uint64_t maj3(uint64_t x, uint64_t y, uint64_t z) { return (x & y) | (x & z) | (y & z); }
static SHA_D uint64_t ch3(uint64_t e, uint64_t f, uint64_t g) { return (e & f) | (~e & g); }
static SHA_D uint64_t big_sigma0(uint64_t a) { return xor3(rotr64(a, 28), rotr64(a, 34), rotr64(a, 39)); }
static SHA_D uint64_t big_sigma1(uint64_t e) { return xor3(rotr64(e, 14), rotr64(e, 18), rotr64(e, 41)); }
static SHA_D uint64_t small_sigma0(uint64_t w) { return xor3(rotr64(w, 1), rotr64(w, 8), w >> 7); }
static SHA_D uint64_t small_sigma1(uint64_t w) { return xor3(rotr64(w, 19), rotr64(w, 61), w >> 6); }

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

// s += x, counting the carry out of bit 63
static SHA_D void add_carry(uint64_t& s, uint32_t& carry, uint64_t x) {
  s += x;
  carry += s < x ? 1u : 0u;
}

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
static SHA_D void sha512_store_all(const Sha512Cols& cols, const uint64_t (&lo)[CQ_SHA256_ADVICE_COLUMNS],
                                   const uint64_t (&hi)[CQ_SHA256_ADVICE_COLUMNS], uint32_t row, std::integer_sequence<uint32_t, I...>) {
  (st(cols.p[I] + row, (lo[I] | hi[I]) ? sha512_encode(lo[I], hi[I]) : Fr::zero()), ...);
}

// One thread per row.  `regions` holds `nregions` entries; rows behind them are written as zero, rows at or behind n not
// at all.  Every index below is guarded by the region kind the chain kernel sets and by the region index itself.
__global__ __launch_bounds__(256) void sha512_expand_kernel(const Sha512Region* __restrict__ regions, uint32_t nregions, uint32_t n,
                                                            uint32_t table_bits, Sha512Cols cols) {
  const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const uint32_t g = row / CQ_SHA512_REGION_ROWS, r = row % CQ_SHA512_REGION_ROWS;
  uint64_t lo[CQ_SHA256_ADVICE_COLUMNS], hi[CQ_SHA256_ADVICE_COLUMNS];
  CQ_UNROLL for (uint32_t i = 0; i < CQ_SHA256_ADVICE_COLUMNS; i++) lo[i] = hi[i] = 0;
  if (g < nregions) {
    const Sha512Region cur = regions[g];
    const uint32_t kind = (uint32_t)cur.meta & 0xffu;
    uint64_t src[CQ_SHA256_SRC_COUNT];
    CQ_UNROLL for (uint32_t i = 0; i < CQ_SHA256_SRC_COUNT; i++) src[i] = 0;
    src[CQ_SHA256_SRC_A] = cur.a;
    src[CQ_SHA256_SRC_E] = cur.e;
    src[CQ_SHA256_SRC_W] = cur.w;
    src[CQ_SHA256_SRC_S0_EVEN] = big_sigma0(cur.a);
    src[CQ_SHA256_SRC_S0_ODD] = maj3(rotr64(cur.a, 28), rotr64(cur.a, 34), rotr64(cur.a, 39));
    src[CQ_SHA256_SRC_S1_EVEN] = big_sigma1(cur.e);
    src[CQ_SHA256_SRC_S1_ODD] = maj3(rotr64(cur.e, 14), rotr64(cur.e, 18), rotr64(cur.e, 41));
    src[CQ_SHA256_SRC_G0_EVEN] = small_sigma0(cur.w);
    src[CQ_SHA256_SRC_G0_ODD] = maj3(rotr64(cur.w, 1), rotr64(cur.w, 8), cur.w >> 7);
    src[CQ_SHA256_SRC_G1_EVEN] = small_sigma1(cur.w);
    src[CQ_SHA256_SRC_G1_ODD] = maj3(rotr64(cur.w, 19), rotr64(cur.w, 61), cur.w >> 6);
    if ((kind & SHA512_RG_F3) && g >= 2) {
      const Sha512Region p1 = regions[g - 1], p2 = regions[g - 2];
      src[CQ_SHA256_SRC_MAJ_EVEN] = xor3(cur.a, p1.a, p2.a);
      src[CQ_SHA256_SRC_MAJ_ODD] = maj3(cur.a, p1.a, p2.a);
      src[CQ_SHA256_SRC_CHP_EVEN] = cur.e ^ p1.e;
      src[CQ_SHA256_SRC_CHP_ODD] = cur.e & p1.e;
      src[CQ_SHA256_SRC_CHQ_EVEN] = ~cur.e ^ p2.e;
      src[CQ_SHA256_SRC_CHQ_ODD] = ~cur.e & p2.e;
      src[CQ_SHA256_SRC_CH] = ch3(cur.e, p1.e, p2.e);
    }
    if ((kind & SHA512_RG_ROUND) && g >= 4) {
      const Sha512Region p1 = regions[g - 1], p2 = regions[g - 2], p3 = regions[g - 3], p4 = regions[g - 4];
      const uint64_t k = SHA512_K_DEV[((uint32_t)cur.meta >> 8) % 80u];
      // T1 = h + Sigma1(e) + Ch(e, f, g) + K + W as a 64-bit sum and the carries out of it
      uint64_t t1 = p4.e;
      uint32_t c1 = 0;
      add_carry(t1, c1, big_sigma1(p1.e)), add_carry(t1, c1, ch3(p1.e, p2.e, p3.e)), add_carry(t1, c1, k), add_carry(t1, c1, cur.w);
      uint64_t se = t1, sa = t1;
      uint32_t ce = c1, ca = c1;
      add_carry(se, ce, p4.a);
      add_carry(sa, ca, big_sigma0(p1.a)), add_carry(sa, ca, maj3(p1.a, p2.a, p3.a));
      src[CQ_SHA256_SRC_K] = k;
      src[CQ_SHA256_SRC_CARRY_E] = ce;
      src[CQ_SHA256_SRC_CARRY_A] = ca;
    }
    if ((kind & SHA512_RG_SCHED) && g >= 16) {
      uint64_t sw = small_sigma1(regions[g - 2].w);
      uint32_t cw = 0;
      add_carry(sw, cw, regions[g - 7].w), add_carry(sw, cw, small_sigma0(regions[g - 15].w)), add_carry(sw, cw, regions[g - 16].w);
      src[CQ_SHA256_SRC_CARRY_W] = cw;
    }
    if ((kind & SHA512_RG_CHAIN) && g >= CQ_SHA512_BLOCK_REGIONS) {
      const Sha512Region h = regions[g - CQ_SHA512_BLOCK_REGIONS], v = regions[g - 4];
      src[CQ_SHA256_SRC_CARRY_A] = h.a + v.a < h.a ? 1u : 0u;
      src[CQ_SHA256_SRC_CARRY_E] = h.e + v.e < h.e ? 1u : 0u;
    }
    sha512_place_all(src, lo, hi, r, table_bits, std::make_integer_sequence<uint32_t, SHA512_NUM_CELLS>{});
  }
  sha512_store_all(cols, lo, hi, row, std::make_integer_sequence<uint32_t, CQ_SHA256_ADVICE_COLUMNS>{});
}

static SHA_D void sha512_put(Sha512Region* p, uint64_t a, uint64_t e, uint64_t w, uint32_t meta) {
  ulonglong2* q = reinterpret_cast<ulonglong2*>(p);
  q[0] = make_ulonglong2(a, e);
  q[1] = make_ulonglong2(w, meta);
}

// a_-4 .. a_-1 = d, c, b, a and e_-4 .. e_-1 = h, g, f, e
static SHA_D void sha512_put_state(Sha512Region* out, const uint64_t (&h)[8], uint32_t chain) {
  sha512_put(out + 0, h[3], h[7], 0, chain);
  sha512_put(out + 1, h[2], h[6], 0, chain);
  sha512_put(out + 2, h[1], h[5], 0, chain | SHA512_RG_F3);
  sha512_put(out + 3, h[0], h[4], 0, chain | SHA512_RG_F3);
}

// Round T0 + I on the 16-word rolling schedule and the state (a .. h), and its region.  I is a compile-time constant, so
// `w` and `s` are only ever indexed by constants and stay in registers; T0, the group's first round, may be a loop variable.
template <bool SCHED, uint32_t I>
static SHA_D void sha512_step(uint64_t (&s)[8], uint64_t (&w)[16], uint32_t t0, Sha512Region* out) {
  if (SCHED) w[I] += small_sigma1(w[(I + 14) & 15]) + w[(I + 9) & 15] + small_sigma0(w[(I + 1) & 15]);
  const uint64_t t1 = s[7] + big_sigma1(s[4]) + ch3(s[4], s[5], s[6]) + SHA512_K_DEV[t0 + I] + w[I];
  const uint64_t t2 = big_sigma0(s[0]) + maj3(s[0], s[1], s[2]);
  s[7] = s[6], s[6] = s[5], s[5] = s[4], s[4] = s[3] + t1;
  s[3] = s[2], s[2] = s[1], s[1] = s[0], s[0] = t1 + t2;
  sha512_put(out + t0 + I, s[0], s[4], w[I], SHA512_RG_ROUND | SHA512_RG_F3 | (SCHED ? SHA512_RG_SCHED : 0) | (t0 + I) << 8);
}
template <bool SCHED, uint32_t... I>
static SHA_D void sha512_steps(uint64_t (&s)[8], uint64_t (&w)[16], uint32_t t0, Sha512Region* out, std::integer_sequence<uint32_t, I...>) {
  (sha512_step<SCHED, I>(s, w, t0, out), ...);
}
// A source of the wired form: a word of the caller's buffer or a word of a final state that an earlier level's launch
// stored.  The host has checked every source against both arrays' lengths.
static SHA_D uint64_t sha512_load(uint32_t s, const uint64_t* words, const uint64_t* digests) {
  return *((s & CQ_SHA512_SOURCE_DIGEST) ? digests + (s & (CQ_SHA512_SOURCE_DIGEST - 1)) : words + s);
}
// The 16 message words of a block.  Unwired, `words` points at them; WIRED, `src` holds their 16 sources.  A fold over
// constant indices, not a loop: `w` is only ever indexed by constants and stays in registers.
template <bool WIRED, uint32_t... I>
static SHA_D void sha512_fetch_all(uint64_t (&w)[16], const uint64_t* words, const uint32_t* src, const uint64_t* digests,
                                   std::integer_sequence<uint32_t, I...>) {
  if constexpr (WIRED)
    ((w[I] = sha512_load(src[I], words, digests)), ...);
  else
    ((w[I] = words[I]), ...);
}
// Word I of the state a wired lane's chain starts from: the variant's own on the sentinel, else a source
template <uint32_t I>
static SHA_D void sha512_fetch_init(uint64_t (&h)[8], uint32_t s, const uint64_t* words, const uint64_t* digests) {
  if (s != CQ_SHA512_SOURCE_IV) h[I] = sha512_load(s, words, digests);
}

// One lane per segment: the compression chain of one message, 80 dependent rounds per block, so the launch is
// latency-bound: one wave per workgroup spreads the segments over the CUs.  Lanes of a wave may differ in their block
// counts and their variants.  The host has checked that every lane's regions lie below n / CQ_SHA512_REGION_ROWS and its
// words inside `words`.
// Unwired (cq_sha512_synthesize_dev): lane i is segment i, its message words lie at words + first_word, and neither
// `sources` nor `init_sources` is looked at.  WIRED (cq_sha512_synthesize_segments_dev): the launch is one level's lanes;
// a lane's segment sits above the variant bit of Sha512Lane::variant, its 16 * blocks sources at sources + first_word and
// its eight initial sources (32 bytes, aligned to 16) at init_sources + 8 * segment; `digests` is read (earlier levels')
// and written (this lane's segment).
template <bool WIRED>
__global__ __launch_bounds__(64) void sha512_chain_kernel(const Sha512Lane* __restrict__ lanes, uint32_t nlanes, const uint64_t* words,
                                                          uint64_t* digests, Sha512Region* __restrict__ regions,
                                                          const uint32_t* __restrict__ sources, const uint32_t* __restrict__ init_sources) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nlanes) return;
  const Sha512Lane lane = lanes[i];
  using Seq16 = std::make_integer_sequence<uint32_t, 16>;
  const uint32_t segment = WIRED ? lane.variant >> 1 : i;
  const uint64_t* iv = SHA512_IV_DEV[lane.variant & 1u];
  uint64_t h[8] = {iv[0], iv[1], iv[2], iv[3], iv[4], iv[5], iv[6], iv[7]};
  if constexpr (WIRED) {
    const uint4* is = reinterpret_cast<const uint4*>(init_sources + 8 * (size_t)segment);
    const uint4 lo = is[0], hi = is[1];
    sha512_fetch_init<0>(h, lo.x, words, digests), sha512_fetch_init<1>(h, lo.y, words, digests);
    sha512_fetch_init<2>(h, lo.z, words, digests), sha512_fetch_init<3>(h, lo.w, words, digests);
    sha512_fetch_init<4>(h, hi.x, words, digests), sha512_fetch_init<5>(h, hi.y, words, digests);
    sha512_fetch_init<6>(h, hi.z, words, digests), sha512_fetch_init<7>(h, hi.w, words, digests);
  }
  Sha512Region* out = regions + lane.first_region;
  const uint64_t* msg = WIRED ? words : words + lane.first_word;
  const uint32_t* src = WIRED ? sources + lane.first_word : nullptr;
  for (uint32_t b = 0; b < lane.blocks; b++, out += CQ_SHA512_BLOCK_REGIONS) {
    sha512_put_state(out, h, b ? SHA512_RG_CHAIN : 0);
    uint64_t w[16], s[8] = {h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7]};
    sha512_fetch_all<WIRED>(w, msg, src, digests, Seq16{});
    if (WIRED) src += 16; else msg += 16;
    sha512_steps<false>(s, w, 0, out + 4, Seq16{});
    for (uint32_t t0 = 16; t0 < 80; t0 += 16) sha512_steps<true>(s, w, t0, out + 4, Seq16{});
    h[0] += s[0], h[1] += s[1], h[2] += s[2], h[3] += s[3];
    h[4] += s[4], h[5] += s[5], h[6] += s[6], h[7] += s[7];
  }
  sha512_put_state(out, h, SHA512_RG_CHAIN);
  uint64_t* d = digests + 8 * (size_t)segment;
  d[0] = h[0], d[1] = h[1], d[2] = h[2], d[3] = h[3], d[4] = h[4], d[5] = h[5], d[6] = h[6], d[7] = h[7];
}

// Validates the description, then queues the upload of the lanes and the message words, the chain launch, the expansion
// and the digests' download on the context's stream, and waits for the stream once.  The staging is pinned; a segment
// synthesis of sha256.hip queued before this call may still copy out of it, so its event is waited for first.
int sha512_synthesize(cq_ctx* c, uint32_t table_bits, const uint32_t* seg_blocks, size_t segments, const uint32_t* seg_variant,
                      const uint64_t* msg_words, uint32_t n, const Sha512Cols& cols, uint64_t* digests_out) {
  const uint64_t max_regions = n / CQ_SHA512_REGION_ROWS;
  uint64_t regions = 0, blocks = 0;
  for (size_t j = 0; j < segments; j++) {
    if (seg_blocks[j] == 0) return c->fail(CQ_ERR_ARG, "sha512: segment " + std::to_string(j) + " has no block");
    if (seg_variant[j] != CQ_SHA512_VARIANT_512 && seg_variant[j] != CQ_SHA512_VARIANT_384)
      return c->fail(CQ_ERR_ARG, "sha512: segment " + std::to_string(j) + " has variant " + std::to_string(seg_variant[j]));
    blocks += seg_blocks[j];
    regions += (uint64_t)seg_blocks[j] * CQ_SHA512_BLOCK_REGIONS + CQ_SHA512_TAIL_REGIONS;
    if (regions > max_regions) return c->fail(CQ_ERR_ARG, "sha512: the segments up to segment " + std::to_string(j) + " do not fit the rows");
  }
  static_assert(sizeof(Sha512Region) == 32 && sizeof(Sha512Lane) == 16, "four words each");
  // lanes, then message words; the digests behind them: every part a multiple of 16 bytes
  const size_t lanes_bytes = segments * sizeof(Sha512Lane), words_bytes = 16 * blocks * sizeof(uint64_t);
  const size_t tables_bytes = lanes_bytes + words_bytes, digests_bytes = 8 * segments * sizeof(uint64_t);
  void *pin, *dev_regions, *dev_tables;
  if (c->sha_staged) CQ_HIP(c, hipEventSynchronize(c->sha_staged));
  CQ_TRY(c->ensure_pinned_sha(tables_bytes + digests_bytes, &pin));
  CQ_TRY(c->ensure_scratch(Scratch::EntryA, regions * sizeof(Sha512Region), &dev_regions));
  CQ_TRY(c->ensure_scratch(Scratch::EntryB, tables_bytes + digests_bytes, &dev_tables));
  Sha512Lane* lanes = (Sha512Lane*)pin;
  uint32_t first_region = 0, first_word = 0;
  for (size_t j = 0; j < segments; j++) {
    lanes[j] = {first_region, seg_blocks[j], first_word, seg_variant[j]};
    first_region += seg_blocks[j] * CQ_SHA512_BLOCK_REGIONS + CQ_SHA512_TAIL_REGIONS;
    first_word += 16 * seg_blocks[j];
  }
  memcpy((char*)pin + lanes_bytes, msg_words, words_bytes);
  CQ_HIP(c, hipMemcpyAsync(dev_tables, pin, tables_bytes, hipMemcpyHostToDevice, c->stream));
  const Sha512Lane* dev_lanes = (const Sha512Lane*)dev_tables;
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
int sha512_synthesize_segments(cq_ctx* c, uint32_t table_bits, const uint32_t* seg_blocks, size_t segments, const uint32_t* seg_variant,
                               const uint32_t* sources, const uint32_t* init_sources, const uint64_t* words_dev, size_t words_len, uint32_t n,
                               const Sha512Cols& cols, uint64_t* digests_dev) {
  const uint64_t max_regions = n / CQ_SHA512_REGION_ROWS;
  uint64_t regions = 0, blocks = 0;
  for (size_t j = 0; j < segments; j++) {
    if (seg_blocks[j] == 0) return c->fail(CQ_ERR_ARG, "sha512: segment " + std::to_string(j) + " has no block");
    if (seg_variant[j] != CQ_SHA512_VARIANT_512 && seg_variant[j] != CQ_SHA512_VARIANT_384)
      return c->fail(CQ_ERR_ARG, "sha512: segment " + std::to_string(j) + " has variant " + std::to_string(seg_variant[j]));
    blocks += seg_blocks[j];
    regions += (uint64_t)seg_blocks[j] * CQ_SHA512_BLOCK_REGIONS + CQ_SHA512_TAIL_REGIONS;
    if (regions > max_regions) return c->fail(CQ_ERR_ARG, "sha512: the segments up to segment " + std::to_string(j) + " do not fit the rows");
  }
  std::vector<uint32_t> level(segments, 0), level_count;
  for (size_t j = 0, at = 0; j < segments; j++) {
    // a source of segment j: "" if it is good, and the segment's level follows a digest's
    auto check = [&](uint32_t s) -> std::string {
      if (s == CQ_SHA512_SOURCE_IV) return " is the initial-value sentinel, which only an initial word can be";
      if (s & CQ_SHA512_SOURCE_DIGEST) {
        const size_t ref = (s & (CQ_SHA512_SOURCE_DIGEST - 1)) >> 3;
        if (ref >= j) return " reads the digest of segment " + std::to_string(ref) + ", which does not come before it";
        if (level[ref] + 1 > level[j]) level[j] = level[ref] + 1;
      } else if (s >= words_len) {
        return " reads word " + std::to_string(s) + " of a buffer of " + std::to_string(words_len);
      }
      return "";
    };
    for (size_t i = 0; init_sources && i < 8; i++) {
      const uint32_t s = init_sources[8 * j + i];
      if (s == CQ_SHA512_SOURCE_IV) continue;
      const std::string bad = check(s);
      if (!bad.empty()) return c->fail(CQ_ERR_ARG, "sha512: segment " + std::to_string(j) + ", initial word " + std::to_string(i) + bad);
    }
    for (size_t t = 0; t < 16 * (size_t)seg_blocks[j]; t++, at++) {
      const std::string bad = check(sources[at]);
      if (!bad.empty()) return c->fail(CQ_ERR_ARG, "sha512: segment " + std::to_string(j) + ", word " + std::to_string(t) + bad);
    }
  }
  for (uint32_t l : level) {
    if (l >= level_count.size()) level_count.resize(l + 1, 0);
    level_count[l]++;
  }
  std::vector<uint32_t> level_first(level_count.size(), 0);
  for (size_t l = 1; l < level_count.size(); l++) level_first[l] = level_first[l - 1] + level_count[l - 1];

  // lanes, sources, initial sources: each a multiple of 16 bytes, so a segment's eight initial sources are aligned for
  // their two 16-byte loads
  const size_t lanes_bytes = segments * sizeof(Sha512Lane), sources_bytes = 16 * blocks * sizeof(uint32_t);
  const size_t init_bytes = 8 * segments * sizeof(uint32_t), tables_bytes = lanes_bytes + sources_bytes + init_bytes;
  void *pin, *dev_regions, *dev_tables;
  if (c->sha_staged) CQ_HIP(c, hipEventSynchronize(c->sha_staged));  // the previous call's copy out of `pin`, before it may move
  CQ_TRY(c->ensure_pinned_sha(tables_bytes, &pin));
  CQ_TRY(c->ensure_scratch(Scratch::EntryA, regions * sizeof(Sha512Region), &dev_regions));
  CQ_TRY(c->ensure_scratch(Scratch::EntryB, tables_bytes, &dev_tables));
  if (!c->sha_staged) CQ_HIP(c, hipEventCreateWithFlags(&c->sha_staged, hipEventDisableTiming));
  Sha512Lane* lanes = (Sha512Lane*)pin;
  std::vector<uint32_t> next = level_first;
  uint32_t first_region = 0, first_source = 0;
  for (size_t j = 0; j < segments; j++) {  // lanes in level order, segments of one level in row order
    lanes[next[level[j]]++] = {first_region, seg_blocks[j], first_source, (uint32_t)j << 1 | seg_variant[j]};
    first_region += seg_blocks[j] * CQ_SHA512_BLOCK_REGIONS + CQ_SHA512_TAIL_REGIONS;
    first_source += 16 * seg_blocks[j];
  }
  memcpy((char*)pin + lanes_bytes, sources, sources_bytes);
  uint32_t* staged_init = (uint32_t*)((char*)pin + lanes_bytes + sources_bytes);
  if (init_sources) memcpy(staged_init, init_sources, init_bytes);
  else std::fill(staged_init, staged_init + 8 * segments, CQ_SHA512_SOURCE_IV);
  CQ_HIP(c, hipMemcpyAsync(dev_tables, pin, tables_bytes, hipMemcpyHostToDevice, c->stream));
  CQ_HIP(c, hipEventRecord(c->sha_staged, c->stream));
  const Sha512Lane* dev_lanes = (const Sha512Lane*)dev_tables;
  const uint32_t* dev_sources = (const uint32_t*)((const char*)dev_tables + lanes_bytes);
  const uint32_t* dev_init = (const uint32_t*)((const char*)dev_sources + sources_bytes);
  for (size_t l = 0; l < level_count.size(); l++) {
    sha512_chain_kernel<true><<<(level_count[l] + 63) / 64, 64, 0, c->stream>>>(dev_lanes + level_first[l], level_count[l], words_dev, digests_dev,
                                                                               (Sha512Region*)dev_regions, dev_sources, dev_init);
    if (hipGetLastError() != hipSuccess) return c->fail(CQ_ERR_HIP, "sha512_chain launch failed");
  }
  sha512_expand_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>((const Sha512Region*)dev_regions, (uint32_t)regions, n, table_bits, cols);
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
  if (!seg_blocks || !seg_variant || !msg_words || !cols_dev || !digests_out || segments == 0 || n > 0x7fffffffull || segments > n)
    return c->fail(CQ_ERR_ARG, "sha512: null array, no segment, or a length out of range");
  if (table_bits < CQ_SHA512_MIN_TABLE_BITS || table_bits > CQ_SHA512_MAX_TABLE_BITS)
    return c->fail(CQ_ERR_ARG, "sha512: table_bits outside the range the pieces fit");
  CQ_HIP(c, hipSetDevice(c->device));
  Sha512Cols sc;
  for (uint32_t i = 0; i < CQ_SHA256_ADVICE_COLUMNS; i++) {
    if (!cols_dev[i]) return c->fail(CQ_ERR_ARG, "sha512: null column");
    sc.p[i] = (Fr*)cols_dev[i];
  }
  return sha512_synthesize(c, table_bits, seg_blocks, segments, seg_variant, msg_words, (uint32_t)n, sc, digests_out);
}

int cq_sha512_synthesize_segments_dev(cq_ctx* c, uint32_t table_bits, const uint32_t* seg_blocks, size_t segments, const uint32_t* seg_variant,
                                      const uint32_t* sources, const uint32_t* init_sources, const uint64_t* words_dev, size_t words_len, size_t n,
                                      uint64_t* const* cols_dev, uint64_t* digests_dev) {
  if (!c) return CQ_ERR_ARG;
  if (!seg_blocks || !seg_variant || !sources || !cols_dev || !digests_dev || segments == 0 || n > 0x7fffffffull || segments > n ||
      (!words_dev && words_len) || words_len > CQ_SHA512_SOURCE_DIGEST)
    return c->fail(CQ_ERR_ARG, "sha512: null array, no segment, or a length out of range");
  if (table_bits < CQ_SHA512_MIN_TABLE_BITS || table_bits > CQ_SHA512_MAX_TABLE_BITS)
    return c->fail(CQ_ERR_ARG, "sha512: table_bits outside the range the pieces fit");
  CQ_HIP(c, hipSetDevice(c->device));
  Sha512Cols sc;
  for (uint32_t i = 0; i < CQ_SHA256_ADVICE_COLUMNS; i++) {
    if (!cols_dev[i]) return c->fail(CQ_ERR_ARG, "sha512: null column");
    sc.p[i] = (Fr*)cols_dev[i];
  }
  return sha512_synthesize_segments(c, table_bits, seg_blocks, segments, seg_variant, sources, init_sources, words_dev, words_len, (uint32_t)n, sc,
                                    digests_dev);
}

}  // extern "C"

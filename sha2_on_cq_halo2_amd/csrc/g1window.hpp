// Regular signed-digit recoding of a scalar for the fixed-window G1 multiplication of g1_fft_windowed (g1fft.hip).
//
// k P for a canonical k < r is computed as  sign * sum_i d_i 8^i P  with EIGHTY-FIVE digits d_i, every one of them ODD and in
// {-7, -5, ..., 5, 7}: there is no zero digit, so every window costs three doublings and ONE addition of a table entry
// +-{1, 3, 5, 7} P in every lane, whatever the scalar -- the control flow of the chain does not depend on a scalar bit.
//   * Such digits exist for an odd scalar only.  r is odd, so one of k and r - k is: an even k is replaced by r - k and the
//     result negated (`flip`; (r - k) P = -k P).  k = 0 becomes r itself, and the chain then ends at r P = the identity.
//   * For an odd m < 2^255 let c = (m + 2^255 - 1) / 2 = (m >> 1) + 2^254, a 255-bit number with bits c_j.  Then
//     m = sum_j (2 c_j - 1) 2^j (j < 255): a string of +-1.  Three of them are one digit: d_i = 2 v_i - 7 with the window
//     v_i = bits [3 i, 3 i + 3) of c.  m < 2^254 gives v_84 = 4 or 5: the top digit is 1 or 3, never negative.
// Plain integer code: compiles for the device and, with __device__ / __forceinline__ defined away, with a host compiler
// (tests/host/g1window_check.cpp checks it against Python integers).
#pragma once
#include <cstdint>
#include "field.hpp"

namespace cq {

constexpr int G1W_BITS = 3;                          // window width: a table of 2^(G1W_BITS - 1) = 4 odd multiples
constexpr int G1W_DIGITS = 255 / G1W_BITS;           // 85
static_assert(G1W_DIGITS * G1W_BITS == 255, "the windows tile the 255 bits of c exactly");

struct G1Recoded {
  uint32_t c[8];   // (m >> 1) + 2^254, m = k or r - k, whichever is odd
  uint32_t flip;   // 1: m = r - k, the product is -(m P)
};

// k: eight words of a canonical scalar, k < r
__device__ __forceinline__ G1Recoded g1w_recode(const uint32_t* k) {
  G1Recoded o;
  o.flip = (k[0] & 1u) ^ 1u;
  const uint32_t mask = 0u - o.flip;
  uint32_t m[8];
  uint64_t borrow = 0;
  CQ_UNROLL for (int i = 0; i < 8; i++) {  // r - k (k < r: no borrow out), taken under the mask
    const uint64_t d = (uint64_t)FrP::MOD[i] - k[i] - borrow;
    borrow = (d >> 32) & 1u;
    m[i] = (k[i] & ~mask) | ((uint32_t)d & mask);
  }
  CQ_UNROLL for (int i = 0; i < 8; i++) o.c[i] = (m[i] >> 1) | (i + 1 < 8 ? m[i + 1] << 31 : 0u);
  o.c[7] |= 1u << 30;  // + 2^254 (m < 2^254: the bit is free)
  return o;
}

// v_i, the window of digit i < G1W_DIGITS (the digit is 2 v_i - 7).  i is the same in every lane (a loop counter): the two
// words the window may straddle are chosen by compares, not by indexing the array at run time.
__device__ __forceinline__ uint32_t g1w_window(const G1Recoded& s, int i) {
  const int bit = G1W_BITS * i, word = bit >> 5, sh = bit & 31;
  uint32_t lo = 0, hi = 0;
  CQ_UNROLL for (int j = 0; j < 8; j++) {
    lo = (word == j) ? s.c[j] : lo;
    hi = (word + 1 == j) ? s.c[j] : hi;
  }
  const uint64_t two = (uint64_t)lo | ((uint64_t)hi << 32);
  return (uint32_t)(two >> sh) & ((1u << G1W_BITS) - 1u);
}
// table index (|d| - 1) / 2 in [0, 4) and sign of the digit d = 2 v - 7
__device__ __forceinline__ uint32_t g1w_index(uint32_t v) { return v >= 4u ? v - 4u : 3u - v; }
__device__ __forceinline__ bool g1w_negative(uint32_t v) { return v < 4u; }

}  // namespace cq

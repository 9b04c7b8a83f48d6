// Square root in a prime field with p = 3 (mod 4) on the lazy 29-bit limb form (field29.hpp): sqrt(a) = a^((p + 1) / 4)
// (`Fq::sqrt`, bn256/fq.rs; the exponent is (p + 1) / 4 because p = 3 mod 4).  The power is a square root only when a is a
// quadratic residue: the caller checks y^2 == a (sqrt_is_root29), as `CurveAffine::from_bytes` does (derive/curve.rs:603-627).
//
// The exponent is a compile-time constant and the same in every lane, so the chain is a fixed-window one: a table of
// a^1 .. a^(2^W - 1) in registers, then per window W squarings and one product with the table entry of the window's digit.
// The digit is wave-uniform (it depends on the loop counter alone), and the entry is chosen by compares over the table's
// registers (sqrt_pick) -- never by indexing a private array at run time, which would put the table into scratch memory.
// W = 4 and BN254's q: 14 products for the table, then 248 squarings and 56 products for the 62 digits below the top one
// (six of them are zero) -- 318 products.  The chain takes its exponent as a template parameter (pow_window29): sqrt2_29.hpp
// runs it with (p - 3) / 4 as well, which has the same digit counts.
//
// Compiles for the device and, with __device__ / __forceinline__ defined away, with a host compiler
// (tests/host/sqrt29_check.cpp); `Trace` sees every intermediate value there and is a no-op in kernels.
#pragma once
#include "field29.hpp"

namespace cq {

// an exponent below 2^256 as eight 32-bit words
struct SqrtExp {
  uint32_t w[8];
};
template <class P>
constexpr SqrtExp make_sqrt_exp() {
  static_assert((P::MOD[0] & 3u) == 3u, "a^((p + 1) / 4) is a square root only for p = 3 (mod 4)");
  uint32_t t[8] = {};
  uint64_t carry = 1;  // p + 1
  for (int i = 0; i < 8; i++) {
    carry += P::MOD[i];
    t[i] = (uint32_t)carry;
    carry >>= 32;
  }
  SqrtExp e{};
  for (int i = 0; i < 8; i++) e.w[i] = (t[i] >> 2) | (i + 1 < 8 ? t[i + 1] << 30 : 0u);  // p < 2^254: no carry out of t
  return e;
}
template <class P>
inline constexpr SqrtExp SQRT_EXP = make_sqrt_exp<P>();
// (p - 3) / 4 = (p + 1) / 4 - 1: a^((p - 3) / 4) is 1 / sqrt(a) up to sign (sqrt2_29.hpp)
template <class P>
constexpr SqrtExp make_inv_sqrt_exp() {
  SqrtExp e = make_sqrt_exp<P>();
  for (int i = 0; i < 8; i++)
    if (e.w[i]-- != 0) break;  // borrow out of a zero word
  return e;
}
template <class P>
inline constexpr SqrtExp INV_SQRT_EXP = make_inv_sqrt_exp<P>();
// The chain's exponent is a type: `word(i)` is a literal once the loops over i are unrolled.
template <class P>
struct ExpSqrt {  // (p + 1) / 4
  static constexpr uint32_t word(int i) { return SQRT_EXP<P>.w[i]; }
};
template <class P>
struct ExpInvSqrt {  // (p - 3) / 4
  static constexpr uint32_t word(int i) { return INV_SQRT_EXP<P>.w[i]; }
};

struct SqrtNoTrace {
  template <class F>
  __device__ __forceinline__ void operator()(const F&) const {}  // a value claimed < 2 p, normalised
  template <class F>
  __device__ __forceinline__ void difference(const F&) const {}  // the root check's y^2 + 8 p - a, claimed < 10 p, normalised
};

// bits [W j, W j + W) of the exponent E; j is wave-uniform (a loop counter), the words are literals after unrolling
template <class E, int W>
__device__ __forceinline__ uint32_t sqrt_exp_digit(int j) {
  static_assert(32 % W == 0, "a digit must not straddle two words");
  const int word = (W * j) >> 5, sh = (W * j) & 31;
  uint32_t e = 0;
  CQ_UNROLL for (int i = 0; i < 8; i++) e = (word == i) ? E::word(i) : e;
  return (e >> sh) & ((1u << W) - 1);
}

// T[d] for a wave-uniform d in [1, 2^W): every entry under the mask of its compare, one v_and_or_b32 per limb with the mask
// in a scalar register.  (Written as `if (d == k) t = T[k]` the struct copies are merged by the optimiser into ONE copy
// from a run-time address, and the whole table moves to scratch memory.)
template <class P, int W>
__device__ __forceinline__ Fp29<P> sqrt_pick(const Fp29<P>* T, uint32_t d) {
  Fp29<P> t = Fp29<P>::zero();
  Fp29<P>::template static_for<1, (1 << W)>([&](auto K) {
    constexpr uint32_t k = decltype(K)::value;
    const uint32_t mask = 0u - (uint32_t)(d == k);
    CQ_UNROLL for (int l = 0; l < 9; l++) t.a[l] |= T[k].a[l] & mask;
  });
  return t;
}

// a^E for a compile-time exponent E < 2^254 (ExpSqrt<P>, ExpInvSqrt<P>), in the R' = 2^261 Montgomery form the operand is in.
//   a: value < 8 p, limbs < 2^30 (a limb-wise sum of up to two normalised values, e.g. x^3 + b).
//   result: normalised, < 2 p.
template <class P, class E, int W = 4, class Trace = SqrtNoTrace>
__device__ __forceinline__ Fp29<P> pow_window29(const Fp29<P>& a, Trace&& tr = Trace()) {
  using F = Fp29<P>;
  constexpr int DIGITS = (254 + W - 1) / W;  // E < 2^254; leading zero digits are skipped below
  F T[1 << W];
  T[1] = a;            // < 8 p, limbs < 2^30
  T[2] = a.sqr();      // 8 * 8 = 64 <= 121, limbs < 2^30  ->  < 2 p, normalised
  tr(T[2]);
  F::template static_for<3, (1 << W)>([&](auto K) {
    constexpr int k = decltype(K)::value;
    T[k] = F::mul(T[k - 1], a);  // 2 * 8 = 16 <= 128, limbs < 2^29 and < 2^30  ->  < 2 p, normalised
    tr(T[k]);
  });
  // the top non-zero digit starts the chain (no squarings of 1)
  int j = DIGITS - 1;
  while (j > 0 && sqrt_exp_digit<E, W>(j) == 0) j--;
  F acc = sqrt_pick<P, W>(T, sqrt_exp_digit<E, W>(j));  // a itself (< 8 p, limbs < 2^30) or a table power (< 2 p)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (j--; j >= 0; j--) {
    CQ_UNROLL for (int s = 0; s < W; s++) {
      acc = acc.sqr();  // 8 * 8 = 64 <= 121 the first time (limbs < 2^30), 2 * 2 = 4 after it  ->  < 2 p, normalised
      tr(acc);
    }
    const uint32_t d = sqrt_exp_digit<E, W>(j);
    if (d) {  // wave-uniform
      acc = F::mul(acc, sqrt_pick<P, W>(T, d));  // 2 * 8 = 16 <= 128, limbs < 2^29 and < 2^30  ->  < 2 p, normalised
      tr(acc);
    }
  }
  return acc;
}

// a^((p + 1) / 4), the candidate square root: operand and result as for pow_window29
template <class P, int W = 4, class Trace = SqrtNoTrace>
__device__ __forceinline__ Fp29<P> sqrt_candidate29(const Fp29<P>& a, Trace&& tr = Trace()) {
  return pow_window29<P, ExpSqrt<P>, W>(a, tr);
}

// y^2 == a (mod p)?   y: normalised, < 2 p (a result of sqrt_candidate29); a: value < 8 p, limbs < 2^30 (its operand).
template <class P, class Trace = SqrtNoTrace>
__device__ __forceinline__ bool sqrt_is_root29(const Fp29<P>& y, const Fp29<P>& a, Trace&& tr = Trace()) {
  using F = Fp29<P>;
  const F y2 = y.sqr();                          // 2 * 2 = 4 <= 121  ->  < 2 p, normalised
  tr(y2);
  const F d = F::template sub<8>(y2, a);         // a < 8 p with limbs < 2^30 (PAD 30), y2 limbs < 2^29: y2 + 8 p - a < 10 p, normalised
  tr.difference(d);
  const F r = d.reduced();                       // 10 * 1 <= 128  ->  < 2 p, normalised
  tr(r);
  return r.is_zero_mod_p();                      // needs < 2 p, normalised
}

}  // namespace cq

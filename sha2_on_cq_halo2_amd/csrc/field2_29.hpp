// Fq2 = Fq[i]/(i^2 + 1) on the lazy 29-bit limbs of field29.hpp, for the G2 kernels (curve2_29.hpp).
//
// Bounds are per component, as multiples of p (the K of field29.hpp); every value is normalised unless said otherwise.
//   * mul(a, b): c0 = a0 b0 + a1 (K p - b1), c1 = a0 b1 + a1 b0, each ONE Fp29::mul2 -- two products and one reduction.
//     Needs Ka Kb + Ka Kb' <= 128 with Kb' the K of the negation (K = Kb): Ka Kb <= 64.  Result < 2 p.
//     A Karatsuba product (3 products, 3 reductions) costs the same 486 limb multiplies as the two mul2() and doubles the
//     operand bounds through (a0 + a1) (b0 + b1), which the XYZZ formulas cannot afford without extra reductions.
//   * sqr(a): c0 = (a0 + a1)(a0 - a1), c1 = 2 a0 a1 -- two products.  Needs 2 Ka * 2 Ka <= 128: Ka <= 5.  Result < 2 p.
//   * mul2(a, b, c, d) = a b + c d: four products per component and one reduction.  Needs the sum of the four bound
//     products (with the negated operands' K) <= 128.  Result < 2 p.
//   * add(): limb-wise (limbs < 2^30, not normalised); sub<K>(a, b) needs b < K p; neg<K>(b) likewise.
#pragma once
#include "field29.hpp"

namespace cq {

struct Fq2_29 {
  Fq29 c0, c1;

  static __device__ __forceinline__ Fq2_29 zero() { return {Fq29::zero(), Fq29::zero()}; }
  static __device__ __forceinline__ Fq2_29 one() { return {Fq29::one(), Fq29::zero()}; }
  __device__ __forceinline__ bool limbs_zero() const { return c0.limbs_zero() && c1.limbs_zero(); }
  // == 0 in Fq2, components normalised and < 2 p
  __device__ __forceinline__ bool is_zero_mod_p() const { return c0.is_zero_mod_p() && c1.is_zero_mod_p(); }
  __device__ __forceinline__ void normalise() {
    c0.normalise();
    c1.normalise();
  }
  __device__ __forceinline__ Fq2_29 operator+(const Fq2_29& o) const { return {c0 + o.c0, c1 + o.c1}; }
  template <uint32_t K, uint32_t PAD = 30>
  static __device__ __forceinline__ Fq2_29 sub(const Fq2_29& x, const Fq2_29& y) {
    return {Fq29::sub<K, PAD>(x.c0, y.c0), Fq29::sub<K, PAD>(x.c1, y.c1)};
  }
  template <uint32_t K>
  static __device__ __forceinline__ Fq2_29 neg(const Fq2_29& y) {
    return {Fq29::neg<K>(y.c0), Fq29::neg<K>(y.c1)};
  }
  // KB: the bound of b (for the negation of b1)
  template <uint32_t KB>
  static __device__ __forceinline__ Fq2_29 mul(const Fq2_29& a, const Fq2_29& b) {
    const Fq29 nb1 = Fq29::neg<KB>(b.c1);
    return {Fq29::mul2(a.c0, b.c0, a.c1, nb1), Fq29::mul2(a.c0, b.c1, a.c1, b.c0)};
  }
  // KA: the bound of a (for a0 - a1)
  template <uint32_t KA>
  __device__ __forceinline__ Fq2_29 sqr() const {
    const Fq29 s = c0 + c1;                      // 2 KA, limbs < 2^30
    const Fq29 d = Fq29::sub<KA>(c0, c1);        // 2 KA
    const Fq29 t = c0 + c0;                      // 2 KA, limbs < 2^30
    Fq2_29 r;
    Fq29::mul_pair(s, d, t, c1, r.c0, r.c1);
    return r;
  }
  // a b + c d; KB, KD: the bounds of b and d (for the negations of b1 and d1)
  template <uint32_t KB, uint32_t KD>
  static __device__ __forceinline__ Fq2_29 mul2(const Fq2_29& a, const Fq2_29& b, const Fq2_29& c, const Fq2_29& d) {
    const Fq29 nb1 = Fq29::neg<KB>(b.c1), nd1 = Fq29::neg<KD>(d.c1);
    uint64_t w[18];
    CQ_UNROLL for (int k = 0; k < 18; k++) w[k] = 0;
    Fq29::mac(w, a.c0, b.c0);
    Fq29::mac(w, a.c1, nb1);
    Fq29::mac(w, c.c0, d.c0);
    Fq29::mac(w, c.c1, nd1);
    Fq2_29 r;
    r.c0 = Fq29::redc(w);
    CQ_UNROLL for (int k = 0; k < 18; k++) w[k] = 0;
    Fq29::mac(w, a.c0, b.c1);
    Fq29::mac(w, a.c1, b.c0);
    Fq29::mac(w, c.c0, d.c1);
    Fq29::mac(w, c.c1, d.c0);
    r.c1 = Fq29::redc(w);
    return r;
  }
  // value < 64 p per component -> < 2 p
  __device__ __forceinline__ Fq2_29 reduced() const { return {c0.reduced(), c1.reduced()}; }
};

}  // namespace cq

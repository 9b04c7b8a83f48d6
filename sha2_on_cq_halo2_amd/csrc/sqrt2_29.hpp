// Square root in Fq2 = Fq[i]/(i^2 + 1) on the lazy 29-bit limbs (field29.hpp, field2_29.hpp), for G2 point decompression:
// `GroupEncoding::from_bytes` for G2Affine (derive/curve.rs:603-627) computes y = (x^3 + b').sqrt() with `Fq2::sqrt`
// (bn256/fq2.rs:344-398, Algorithm 9 of eprint 2012/685) and negates it when ysign ^ (parity of the canonical y.c0).
//
// What is computed here is that DECODED y, not the algorithm: Algorithm 9 costs two 254-bit exponentiations in Fq2 (about
// 1 700 Fq products); the route below needs two in Fq and no inversion.  With a = a0 + a1 i:
//     n = a0^2 + a1^2 (the norm),  s = n^((q + 1) / 4);  a is a square in Fq2 exactly when s^2 == n  (`Fq2::legendre` is the
//         norm's Legendre symbol, fq2.rs:157-159; n = 0 only for a = 0 because -1 is a non-residue of Fq)
//     d = (a0 + s) / 2, or (a0 - s) / 2 where that is 0;   w = d^((q - 3) / 4),  c = w d
//     -1 is a non-residue, so c^2 is d or -d, and c w = d^((q - 1) / 2) is 1 or -1 accordingly:
//         c^2 ==  d:  y = ( c,  a1 w / 2)      (2 c y1 = a1 c w = a1;  c^2 - y1^2 = d - a1^2 / (4 d) = a0)
//         c^2 == -d:  y = (-a1 w / 2,  c)      (2 y0 c = -a1 w c = a1;  y0^2 - c^2 = -a1^2 / (4 d) + d = a0)
//     using 4 d^2 - a1^2 = 4 a0 d, which holds for either choice of d.
// Both outcomes cost the same products and the result is selected under masks: no wave pays a third exponentiation because
// of one lane.  Which of +-y comes out matters in one case only: a root with y.c0 == 0 has parity 0 either way, so the
// decoded point is the algorithm's root with the sign bit clear and its negative with it set.  That is the case of a REAL
// operand whose a0 is a non-residue, where Algorithm 9 returns (0, a0^((q + 1) / 4)).  Here a1 == 0 gives n = a0^2 and
// s = +-a0 -- the residue of the two -- so a0 + s == 0 exactly for such an operand (and for no other: a0 + s = 0 forces
// a1 = 0), d = a0, c = a0^((q + 1) / 4) and c^2 = -d: the same (0, c).  Everywhere else the parity rule fixes the result.
// (tests/test_serde_g2_cpu.py compares with a literal restatement of Algorithm 9 on every class of operand.)
//
// Cost: 2 + 2 + 318 + 2 + 3 + 318 + 5 = 650 Fq products (the reductions of a0 and a1; the norm as one two-product sum; the
// first chain; s^2 and its reduced difference; the two halvings and a1 / 2; the second chain; c, c^2, its reduced
// difference, a1 w / 2 and its reduced negation) and one more for the parity of the canonical y.c0: 651.  The two chains
// run one after the other: one table of 15 powers is live at a time.
//
// Compiles for the device and, with __device__ / __forceinline__ defined away, with a host compiler
// (tests/host/sqrt2_29_check.cpp); `Trace` sees every intermediate value there and is a no-op in kernels.
#pragma once
#include "field2_29.hpp"
#include "sqrt29.hpp"

namespace cq {

struct Sqrt2NoTrace : SqrtNoTrace {
  using SqrtNoTrace::operator();  // a value claimed < 2 p, normalised
  template <class F>
  __device__ __forceinline__ void below4(const F&) const {}  // a value claimed < 4 p, normalised (a sub<2> of two values < 2 p)
  template <class F>
  __device__ __forceinline__ void negated(const F&) const {}  // a neg<2>: claimed <= 2 p (2 p itself for 0), normalised
};

// 1 / 2 in the R' = 2^261 Montgomery form: 2^260 mod q
struct Sqrt2Consts {
  uint32_t half[9];
};
constexpr Sqrt2Consts make_sqrt2_consts() {
  Sqrt2Consts c{};
  pow2_mod_p29<FqP>(260, c.half);
  return c;
}
inline constexpr Sqrt2Consts SQRT2_CONSTS = make_sqrt2_consts();

// v under the mask m (all ones or zero), else u
__device__ __forceinline__ Fq29 sqrt2_select(const Fq29& u, const Fq29& v, uint32_t m) {
  Fq29 r;
  CQ_UNROLL for (int l = 0; l < 9; l++) r.a[l] = (u.a[l] & ~m) | (v.a[l] & m);
  return r;
}

// A square root of a, and whether a has one.
//   a: each component a value < 8 q with limbs < 2^30 (e.g. x^3 + b' as a limb-wise sum), R' Montgomery form.
//   y: each component normalised and < 2 q; y^2 == a when the function returns true, unspecified otherwise.
template <int W = 4, class Trace = Sqrt2NoTrace>
__device__ __forceinline__ bool fq2_sqrt29(const Fq2_29& a, Fq2_29& y, Trace&& tr = Trace()) {
  using F = Fq29;
  F half;
  CQ_UNROLL for (int l = 0; l < 9; l++) half.a[l] = SQRT2_CONSTS.half[l];  // < q, normalised
  const F a0 = F::mul(a.c0, F::one());          // 8 * 1 <= 128, limbs < 2^30 and < 2^29  ->  < 2 q, normalised
  tr(a0);
  const F a1 = F::mul(a.c1, F::one());          // likewise
  tr(a1);
  const F n = F::mul2(a0, a0, a1, a1);          // 2 * 2 + 2 * 2 = 8 <= 128, all normalised  ->  < 2 q
  tr(n);
  const F s = pow_window29<FqP, ExpSqrt<FqP>, W>(n, tr);  // operand < 2 q <= 8 q  ->  < 2 q, normalised
  const F s2 = s.sqr();                          // 2 * 2 = 4 <= 121  ->  < 2 q
  tr(s2);
  const F e = F::sub<2>(s2, n);                  // n < 2 q, limbs < 2^29: s2 + 2 q - n < 4 q, normalised
  tr.below4(e);
  const F er = e.reduced();                      // 4 * 1 <= 128  ->  < 2 q
  tr(er);
  const bool square = er.is_zero_mod_p();        // needs < 2 q, normalised
  const F dps = a0 + s;                          // limb-wise: < 4 q, limbs < 2^30
  const F dms = F::sub<2>(a0, s);                // s < 2 q: a0 + 2 q - s < 4 q, normalised
  tr.below4(dms);
  const F dp = F::mul(dps, half);                // 4 * 1 <= 128, limbs < 2^30 and < 2^29  ->  (a0 + s) / 2 < 2 q, normalised
  tr(dp);
  const F dm = F::mul(dms, half);                // 4 * 1 <= 128  ->  (a0 - s) / 2 < 2 q
  tr(dm);
  const F h = F::mul(a1, half);                  // 2 * 1 <= 128  ->  a1 / 2 < 2 q   (before the chain: a1 dies here)
  tr(h);
  const F d = sqrt2_select(dp, dm, 0u - (uint32_t)dp.is_zero_mod_p());  // < 2 q, normalised
  const F w = pow_window29<FqP, ExpInvSqrt<FqP>, W>(d, tr);             // operand < 2 q <= 8 q  ->  < 2 q, normalised
  const F c = F::mul(w, d);                      // 2 * 2 = 4 <= 128  ->  < 2 q
  tr(c);
  const F c2 = c.sqr();                          // 4 <= 121  ->  < 2 q
  tr(c2);
  const F g = F::sub<2>(c2, d);                  // d < 2 q: c2 + 2 q - d < 4 q, normalised
  tr.below4(g);
  const F gr = g.reduced();                      // 4 * 1 <= 128  ->  < 2 q
  tr(gr);
  const F t = F::mul(h, w);                      // 2 * 2 = 4 <= 128  ->  a1 w / 2 < 2 q
  tr(t);
  const F nt = F::neg<2>(t);                     // t < 2 q: 2 q - t in (0, 2 q], normalised
  tr.negated(nt);
  const F ntr = nt.reduced();                    // 2 * 1 <= 128 (holds for 2 q itself)  ->  < 2 q
  tr(ntr);
  const uint32_t plus = 0u - (uint32_t)gr.is_zero_mod_p();  // c^2 == d
  y.c0 = sqrt2_select(ntr, c, plus);
  y.c1 = sqrt2_select(c, t, plus);
  return square;
}

// The y of `from_bytes` for x^3 + b' = a and the sign bit `ysign` (0 or 1): the root above, negated when
// ysign ^ (parity of the canonical y.c0).  Operand as for fq2_sqrt29.  y: components normalised and <= 2 q (2 q itself
// only as the negation of 0), ready for to_mont256().  Returns false when a is not a square.
template <int W = 4, class Trace = Sqrt2NoTrace>
__device__ __forceinline__ bool fq2_decoded_y29(const Fq2_29& a, uint32_t ysign, Fq2_29& y, Trace&& tr = Trace()) {
  using F = Fq29;
  Fq2_29 r;
  const bool square = fq2_sqrt29<W>(a, r, tr);
  // the parity is that of the INTEGER y.c0: a product with the literal 1 divides R' out (as in g1_decompress_kernel)
  F lit1 = F::zero();
  lit1.a[0] = 1;
  const F yc = F::mul(r.c0, lit1);               // 2 * 1 <= 128  ->  y.c0 itself, < 2 q, normalised
  tr(yc);
  uint32_t o[8];
  yc.pack(o);                                    // < 2 q < 2^256
  Fq::cond_sub_p(o, 0);                          // canonical
  const uint32_t flip = 0u - ((o[0] & 1u) ^ ysign);
  const F n0 = F::neg<2>(r.c0), n1 = F::neg<2>(r.c1);  // < 2 q each: in (0, 2 q], normalised
  tr.negated(n0);
  tr.negated(n1);
  y.c0 = sqrt2_select(r.c0, n0, flip);
  y.c1 = sqrt2_select(r.c1, n1, flip);
  return square;
}

}  // namespace cq

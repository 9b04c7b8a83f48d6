// BN254 G2 group law on Fq2 over the lazy 29-bit limbs (field2_29.hpp) for the G2 kernels (msm_g2.hip).
//
// Same XYZZ formulas as curve29.hpp (madd-2008-s, add-2008-s, dbl-2008-s-1; a = 0, so the twist's b' never enters), with a
// simpler invariant than G1's, because an Fq2 square doubles its operand's bound:
//     x, y, zz, zzz < 2 p per component, limbs normalised;  identity <=> all limbs of zz are zero.
// x3 comes out of the formulas below 8 p and is reduced once (one product with 1 per component).  The bound of every
// intermediate is given in the comments (K, per component); field2_29.hpp lists what each operation needs.
#pragma once
#include "curve2.hpp"
#include "curve29.hpp"
#include "field2_29.hpp"

namespace cq {

using F2 = Fq2_29;

struct XYZZ2_29 {
  F2 x, y, zz, zzz;
  static __device__ __forceinline__ XYZZ2_29 identity() { return {F2::zero(), F2::zero(), F2::zero(), F2::zero()}; }
  __device__ __forceinline__ bool is_identity() const { return zz.limbs_zero(); }
};

// affine point in R' form (x, y < 2 p); identity = all limbs zero
struct Affine2_29 {
  F2 x, y;
  __device__ __forceinline__ bool is_identity() const { return x.limbs_zero() && y.limbs_zero(); }
};

// library-internal memory form of an XYZZ point: 8 x (8 x u32) R'-form values < 2 p < 2^256, 256 bytes
struct XYZZ2 {
  uint32_t w[64];
};

// ---- memory <-> registers ---------------------------------------------------------------------------------------
// a G2Affine in the reference's R = 2^256 Montgomery form (one product per coordinate component; 0 stays 0)
static __device__ __forceinline__ Affine2_29 load_affine2_29(const G2Affine* p) {
  const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
  uint32_t w[8];
  Fq29 f;
  CQ_UNROLL for (int i = 0; i < 9; i++) f.a[i] = CONSTS29<FqP>.from256[i];
  Fq29 c[4];
  CQ_UNROLL for (int k = 0; k < 4; k++) {
    ld8(q + 8 * k, w);
    c[k] = Fq29::mul(Fq29::unpack(w), f);
  }
  return {{c[0], c[1]}, {c[2], c[3]}};
}
static __device__ __forceinline__ XYZZ2_29 load_xyzz2_29(const XYZZ2* p) {
  uint32_t w[8];
  Fq29 c[8];
  CQ_UNROLL for (int k = 0; k < 8; k++) {
    ld8(p->w + 8 * k, w);
    c[k] = Fq29::unpack(w);
  }
  return {{c[0], c[1]}, {c[2], c[3]}, {c[4], c[5]}, {c[6], c[7]}};
}
static __device__ __forceinline__ void store_xyzz2_29(XYZZ2* p, const XYZZ2_29& v) {
  uint32_t w[8];
  const Fq29* c[8] = {&v.x.c0, &v.x.c1, &v.y.c0, &v.y.c1, &v.zz.c0, &v.zz.c1, &v.zzz.c0, &v.zzz.c1};
  CQ_UNROLL for (int k = 0; k < 8; k++) {
    c[k]->pack(w);
    st8(p->w + 8 * k, w);
  }
}

// ---- group law --------------------------------------------------------------------------------------------------
// 2 * (ax, ay), affine (x, y < 2 p)
static __device__ __forceinline__ XYZZ2_29 xyzz2_dbl_affine(const Affine2_29& a) {
  if (a.is_identity()) return XYZZ2_29::identity();
  F2 u = a.y + a.y;                                   // < 4
  u.normalise();
  const F2 v = u.sqr<4>();                            // 2
  const F2 w = F2::mul<2>(u, v);                      // 4 * 2 * 2 = 16 -> 2
  const F2 s = F2::mul<2>(a.x, v);                    // 2
  const F2 x2 = a.x.sqr<2>();                         // 2
  F2 m = x2 + x2 + x2;                                // < 6
  m.normalise();
  const F2 x3 = F2::sub<4>(F2::mul<6>(m, m), s + s).reduced();  // 6 * 6 * 2 = 72; < 6 -> 2
  // m (s - x3) - w y: 6 * 4 * 2 + 2 * 2 * 2 = 56
  const F2 y3 = F2::mul2<4, 2>(m, F2::sub<2>(s, x3), w, F2::neg<2>(a.y));
  return {x3, y3, v, w};
}

static __device__ __forceinline__ XYZZ2_29 xyzz2_dbl(const XYZZ2_29& p) {
  if (p.is_identity()) return XYZZ2_29::identity();
  F2 u = p.y + p.y;                                   // < 4
  u.normalise();
  const F2 v = u.sqr<4>();                            // 2
  const F2 w = F2::mul<2>(u, v);                      // 2
  const F2 s = F2::mul<2>(p.x, v);                    // 2
  const F2 x2 = p.x.sqr<2>();                         // 2
  F2 m = x2 + x2 + x2;                                // < 6
  m.normalise();
  const F2 x3 = F2::sub<4>(F2::mul<6>(m, m), s + s).reduced();
  const F2 y3 = F2::mul2<4, 2>(m, F2::sub<2>(s, x3), w, F2::neg<2>(p.y));
  return {x3, y3, F2::mul<2>(v, p.zz), F2::mul<2>(w, p.zzz)};
}

// acc += a, complete (identity operands, a == acc, a == -acc)
static __device__ __forceinline__ void xyzz2_add_affine(XYZZ2_29& acc, const Affine2_29& a) {
  if (a.is_identity()) return;
  if (acc.is_identity()) {
    acc = {a.x, a.y, F2::one(), F2::one()};
    return;
  }
  const F2 u2 = F2::mul<2>(a.x, acc.zz);              // 2
  const F2 s2 = F2::mul<2>(a.y, acc.zzz);             // 2
  const F2 p = F2::sub<2>(u2, acc.x);                 // < 4
  const F2 r = F2::sub<2>(s2, acc.y);                 // < 4
  const F2 pp = p.sqr<4>();                           // 2
  const F2 rr = r.sqr<4>();                           // 2
  if (pp.is_zero_mod_p()) {                           // same x: doubling or cancellation
    if (rr.is_zero_mod_p()) acc = xyzz2_dbl_affine(a);
    else acc = XYZZ2_29::identity();
    return;
  }
  const F2 ppp = F2::mul<2>(p, pp);                   // 4 * 2 * 2 = 16 -> 2
  const F2 q = F2::mul<2>(acc.x, pp);                 // 2
  const F2 x3 = F2::sub<6, 31>(rr, ppp + q + q).reduced();  // subtrahend < 6, limbs < 3 * 2^29; < 8 -> 2
  // r (q - x3) - y1 ppp: 4 * 4 * 2 + 2 * 2 * 2 = 40
  const F2 y3 = F2::mul2<4, 2>(r, F2::sub<2>(q, x3), F2::neg<2>(acc.y), ppp);
  acc.x = x3;
  acc.y = y3;
  acc.zz = F2::mul<2>(acc.zz, pp);
  acc.zzz = F2::mul<2>(acc.zzz, ppp);
}

// acc += b, complete
static __device__ __forceinline__ void xyzz2_add(XYZZ2_29& acc, const XYZZ2_29& b) {
  if (b.is_identity()) return;
  if (acc.is_identity()) {
    acc = b;
    return;
  }
  const F2 u1 = F2::mul<2>(acc.x, b.zz);
  const F2 u2 = F2::mul<2>(b.x, acc.zz);
  const F2 s1 = F2::mul<2>(acc.y, b.zzz);
  const F2 s2 = F2::mul<2>(b.y, acc.zzz);
  const F2 p = F2::sub<2>(u2, u1);                    // < 4
  const F2 r = F2::sub<2>(s2, s1);                    // < 4
  const F2 pp = p.sqr<4>();
  const F2 rr = r.sqr<4>();
  if (pp.is_zero_mod_p()) {
    if (rr.is_zero_mod_p()) acc = xyzz2_dbl(acc);
    else acc = XYZZ2_29::identity();
    return;
  }
  const F2 ppp = F2::mul<2>(p, pp);
  const F2 q = F2::mul<2>(u1, pp);
  const F2 x3 = F2::sub<6, 31>(rr, ppp + q + q).reduced();
  const F2 y3 = F2::mul2<4, 2>(r, F2::sub<2>(q, x3), F2::neg<2>(s1), ppp);
  acc.x = x3;
  acc.y = y3;
  acc.zz = F2::mul<2>(F2::mul<2>(acc.zz, b.zz), pp);
  acc.zzz = F2::mul<2>(F2::mul<2>(acc.zzz, b.zzz), ppp);
}

// canonical R = 2^256 Montgomery form of a component (< 64 p)
static __device__ __forceinline__ Fq2 to_mont256_2(const F2& v) { return {v.c0.to_mont256(), v.c1.to_mont256()}; }

// Jacobian representative (X ZZ, Y ZZZ, ZZ) in the reference's layout
static __device__ __forceinline__ G2Jac xyzz2_to_jac(const XYZZ2_29& v) {
  if (v.is_identity()) return G2Jac::identity();
  return {to_mont256_2(F2::mul<2>(v.x, v.zz)), to_mont256_2(F2::mul<2>(v.y, v.zzz)), to_mont256_2(v.zz)};
}

}  // namespace cq

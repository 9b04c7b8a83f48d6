// BN254 G2 = E'(Fq2): y^2 = x^3 + 3/(9+i) (bn256/curve.rs:85-129) on field.hpp's Fq, for the host side (window folds,
// normalisation, the fixed-base table) and the per-lane normalisation of the SRS kernel.
//
// Fq2 = Fq[i]/(i^2 + 1).  Layouts match halo2curves' raw (SerdeObject) form: affine = {x.c0, x.c1, y.c0, y.c1}, 16 x u64
// of R = 2^256 Montgomery limbs with (0, 0) = identity; Jacobian = {x, y, z} 24 x u64 with z = 0 = identity -- the G1
// layouts of curve.hpp with every coordinate doubled.  The device hot path uses curve2_29.hpp instead.
#pragma once
#include "curve.hpp"

namespace cq {

struct alignas(16) Fq2 {
  Fq c0, c1;
  static CQ_HD Fq2 zero() { return {Fq::zero(), Fq::zero()}; }
  static CQ_HD Fq2 one() { return {Fq::one(), Fq::zero()}; }
  CQ_HD bool is_zero() const { return c0.is_zero() && c1.is_zero(); }
  CQ_HD bool operator==(const Fq2& b) const { return c0 == b.c0 && c1 == b.c1; }
  CQ_HD Fq2 operator+(const Fq2& b) const { return {c0 + b.c0, c1 + b.c1}; }
  CQ_HD Fq2 operator-(const Fq2& b) const { return {c0 - b.c0, c1 - b.c1}; }
  CQ_HD Fq2 neg() const { return {c0.neg(), c1.neg()}; }
  CQ_HD Fq2 dbl() const { return *this + *this; }
  // Karatsuba: 3 products
  CQ_HD Fq2 operator*(const Fq2& b) const {
    const Fq v0 = c0 * b.c0, v1 = c1 * b.c1;
    return {v0 - v1, (c0 + c1) * (b.c0 + b.c1) - v0 - v1};
  }
  // (a + b i)^2 = (a + b)(a - b) + 2 a b i: 2 products
  CQ_HD Fq2 sqr() const { return {(c0 + c1) * (c0 - c1), (c0 * c1).dbl()}; }
  // (a + b i)^-1 = (a - b i) / (a^2 + b^2): one Fq inversion; 0 -> 0
  CQ_HD Fq2 inv() const {
    const Fq t = (c0.sqr() + c1.sqr()).inv();
    return {c0 * t, (c1 * t).neg()};
  }
  static CQ_HD Fq2 from_limbs64(const uint64_t* s) { return {Fq::from_limbs64(s), Fq::from_limbs64(s + 4)}; }
  CQ_HD void to_limbs64(uint64_t* d) const {
    c0.to_limbs64(d);
    c1.to_limbs64(d + 4);
  }
};

struct alignas(16) G2Affine {
  Fq2 x, y;
  CQ_HD bool is_identity() const { return x.is_zero() && y.is_zero(); }
  static CQ_HD G2Affine identity() { return {Fq2::zero(), Fq2::zero()}; }
};
static_assert(sizeof(G2Affine) == 128, "G2 affine is 16 x u64");

struct alignas(16) G2Jac {
  Fq2 x, y, z;
  static CQ_HD G2Jac identity() { return {Fq2::zero(), Fq2::zero(), Fq2::zero()}; }
  CQ_HD bool is_identity() const { return z.is_zero(); }
};
static_assert(sizeof(G2Jac) == 192, "G2 Jacobian is 24 x u64");

// the twist's b' = 3 / (9 + i)
static inline Fq2 g2_b() {
  const Fq2 xi = {Fq::from_u64(9), Fq::one()};
  return Fq2{Fq::from_u64(3), Fq::zero()} * xi.inv();
}

// generator (bn256/curve.rs:100-129), canonical limbs x.c0, x.c1, y.c0, y.c1
static inline G2Affine g2_generator() {
  static const uint64_t raw[4][4] = {
      {0x46DEBD5CD992F6EDull, 0x674322D4F75EDADDull, 0x426A00665E5C4479ull, 0x1800DEEF121F1E76ull},
      {0x97E485B7AEF312C2ull, 0xF1AA493335A9E712ull, 0x7260BFB731FB5D25ull, 0x198E9393920D483Aull},
      {0x4CE6CC0166FA7DAAull, 0xE3D1E7690C43D37Bull, 0x4AAB71808DCB408Full, 0x12C85EA5DB8C6DEBull},
      {0x55ACDADCD122975Bull, 0xBC4B313370B38EF3ull, 0xEC9E99AD690C3395ull, 0x090689D0585FF075ull}};
  Fq c[4];
  for (int k = 0; k < 4; k++) {
    U256 u;
    for (int j = 0; j < 4; j++) {
      u.l[2 * j] = (uint32_t)raw[k][j];
      u.l[2 * j + 1] = (uint32_t)(raw[k][j] >> 32);
    }
    c[k] = Fq::from_canonical(u);
  }
  return {{c[0], c[1]}, {c[2], c[3]}};
}

// y^2 == x^3 + b' (the identity counts as on the curve, as for G1's RawBytes reads)
static inline bool g2_on_curve(const G2Affine& p, const Fq2& b) {
  if (p.is_identity()) return true;
  return p.y.sqr() == p.x.sqr() * p.x + b;
}

// ---- Jacobian group law (a = 0): the G1 formulas of curve.hpp over Fq2 ----
static CQ_HD G2Jac g2_jac_dbl(const G2Jac& p) {
  if (p.is_identity() || p.y.is_zero()) return G2Jac::identity();
  const Fq2 a = p.x.sqr(), b = p.y.sqr(), c = b.sqr();
  const Fq2 d = ((p.x + b).sqr() - a - c).dbl();
  const Fq2 e = a.dbl() + a;
  const Fq2 f = e.sqr();
  const Fq2 x3 = f - d.dbl();
  const Fq2 y3 = e * (d - x3) - c.dbl().dbl().dbl();
  return {x3, y3, (p.y * p.z).dbl()};
}

static CQ_HD G2Jac g2_jac_add(const G2Jac& p, const G2Jac& q) {
  if (p.is_identity()) return q;
  if (q.is_identity()) return p;
  const Fq2 z1z1 = p.z.sqr(), z2z2 = q.z.sqr();
  const Fq2 u1 = p.x * z2z2, u2 = q.x * z1z1;
  const Fq2 s1 = p.y * q.z * z2z2, s2 = q.y * p.z * z1z1;
  if (u1 == u2) {
    if (s1 == s2) return g2_jac_dbl(p);
    return G2Jac::identity();
  }
  const Fq2 h = u2 - u1, r = s2 - s1;
  const Fq2 hh = h.sqr(), hhh = h * hh, v = u1 * hh;
  const Fq2 x3 = r.sqr() - hhh - v.dbl();
  const Fq2 y3 = r * (v - x3) - s1 * hhh;
  return {x3, y3, p.z * q.z * h};
}

static CQ_HD G2Jac g2_jac_neg(const G2Jac& p) { return {p.x, p.y.neg(), p.z}; }

static CQ_HD G2Jac g2_jac_from_affine(const G2Affine& a) {
  if (a.is_identity()) return G2Jac::identity();
  return {a.x, a.y, Fq2::one()};
}

static CQ_HD G2Affine g2_jac_to_affine(const G2Jac& p) {
  if (p.is_identity()) return G2Affine::identity();
  const Fq2 zi = p.z.inv(), zi2 = zi.sqr();
  return {p.x * zi2, p.y * zi2 * zi};
}

static inline G2Jac g2_jac_from_limbs64(const uint64_t* s) {
  return {Fq2::from_limbs64(s), Fq2::from_limbs64(s + 8), Fq2::from_limbs64(s + 16)};
}
static inline void g2_jac_to_limbs64(const G2Jac& p, uint64_t* d) {
  p.x.to_limbs64(d);
  p.y.to_limbs64(d + 8);
  p.z.to_limbs64(d + 16);
}

}  // namespace cq

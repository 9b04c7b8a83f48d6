// SerdeFormat::Processed on the device: point decompression / compression (derive/curve.rs:603-646) for G1 and G2 and the
// canonical scalar encodings (helpers.rs:68-91), with their C entry points.  The params, proving-key and G2 SRS readers
// built on them live next to their raw twins (capi_msm.hip, pk.hip, capi_g2.hip).
#include <cstdint>
#include <string>
#include "ctx.hpp"
#include "serde.hpp"
#include "sqrt29.hpp"
#include "sqrt2_29.hpp"

namespace cq {
namespace {

// r2 = 2^522 mod q: mul(x, r2) takes a canonical x to its R' = 2^261 Montgomery form x R';  b = 3 R' mod q: the curve's
// constant in that form
struct SerdeConsts {
  uint32_t r2[9];
  uint32_t b[9];
};
// out = u + v mod q for canonical 29-bit limb values
constexpr void add_mod_q29(const uint32_t* u, const uint32_t* v, uint32_t* out) {
  uint32_t s[9] = {}, t[9] = {};
  uint32_t carry = 0, borrow = 0;
  for (int i = 0; i < 9; i++) {
    const uint32_t x = u[i] + v[i] + carry;  // < 2^30 + 1
    s[i] = i < 8 ? (x & 0x1fffffffu) : x;
    carry = i < 8 ? (x >> 29) : 0;
  }
  for (int i = 0; i < 9; i++) {  // t = s - q
    const uint32_t sub_ = Fq::p29(i) + borrow;
    if (s[i] >= sub_) {
      t[i] = s[i] - sub_;
      borrow = 0;
    } else {
      t[i] = s[i] + (1u << 29) - sub_;
      borrow = 1;
    }
  }
  for (int i = 0; i < 9; i++) out[i] = borrow ? s[i] : t[i];  // s < 2 q
}
constexpr SerdeConsts make_serde_consts() {
  SerdeConsts c{};
  pow2_mod_p29<FqP>(522, c.r2);
  uint32_t one[9] = {}, two[9] = {};
  pow2_mod_p29<FqP>(261, one);
  pow2_mod_p29<FqP>(262, two);
  add_mod_q29(one, two, c.b);
  return c;
}
constexpr SerdeConsts SERDE_CONSTS = make_serde_consts();

// v 2^e mod q for a canonical v in 29-bit limbs, by repeated doubling
constexpr void shl_mod_q29(const uint32_t* v, int e, uint32_t* out) {
  uint32_t t[9] = {};
  for (int i = 0; i < 9; i++) t[i] = v[i];
  for (int s = 0; s < e; s++) {
    uint32_t d[9] = {};
    add_mod_q29(t, t, d);
    for (int i = 0; i < 9; i++) t[i] = d[i];
  }
  for (int i = 0; i < 9; i++) out[i] = t[i];
}
// four 64-bit words (little-endian) -> nine 29-bit limbs
constexpr void limbs29_of_words64(const uint64_t* w, uint32_t* out) {
  for (int i = 0; i < 9; i++) {
    const int bit = 29 * i, k = bit >> 6, sh = bit & 63;
    uint64_t x = w[k] >> sh;
    if (sh > 35 && k + 1 < 4) x |= w[k + 1] << (64 - sh);
    out[i] = (uint32_t)(x & 0x1fffffffu);
  }
}
// the twist's b' = 3 / (9 + i) (bn256/curve.rs:85-98, canonical words) in the R' = 2^261 Montgomery form
struct Serde2Consts {
  uint32_t b0[9], b1[9];
};
constexpr Serde2Consts make_serde2_consts() {
  constexpr uint64_t B0[4] = {0x3267e6dc24a138e5ull, 0xb5b4c5e559dbefa3ull, 0x81be18991be06ac3ull, 0x2b149d40ceb8aaaeull};
  constexpr uint64_t B1[4] = {0xe4a2bd0685c315d2ull, 0xa74fa084e52d1852ull, 0xcd2cafadeed8fdf4ull, 0x009713b03af0fed4ull};
  Serde2Consts c{};
  uint32_t t[9] = {};
  limbs29_of_words64(B0, t);
  shl_mod_q29(t, 261, c.b0);
  limbs29_of_words64(B1, t);
  shl_mod_q29(t, 261, c.b1);
  return c;
}
constexpr Serde2Consts SERDE2_CONSTS = make_serde2_consts();

__device__ __forceinline__ void ld8(const void* p, uint32_t* w) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}
__device__ __forceinline__ void st8(void* p, const uint32_t* w) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(w[0], w[1], w[2], w[3]);
  q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
template <class P>
__device__ __forceinline__ bool below_modulus(const uint32_t* w) {
  uint64_t br = 0;  // borrow of w - p: set exactly when w < p
  CQ_UNROLL for (int i = 0; i < 8; i++) br = (((uint64_t)w[i] - P::MOD[i] - br) >> 32) & 1;
  return br != 0;
}
__device__ __forceinline__ void report(uint32_t i, uint32_t* count, uint32_t* first) {
  atomicAdd(count, 1u);
  atomicMin(first, i);
}

// CurveAffine::from_bytes (derive/curve.rs:603-627).  One point per lane: about 330 dependent Fq products, no memory
// traffic to speak of and nothing shared between lanes.
__global__ void __launch_bounds__(256) g1_decompress_kernel(const uint8_t* __restrict__ in, uint32_t n, G1Affine* __restrict__ out,
                                                            uint32_t* __restrict__ count, uint32_t* __restrict__ first) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8];
  ld8(in + (size_t)i * 32, w);
  const uint32_t ysign = w[7] >> 31;  // bit 7 of byte 31
  w[7] &= 0x7fffffffu;
  if (!below_modulus<FqP>(w)) {  // `Fq::from_bytes` fails on a non-canonical x (bit 254 set is always one: q < 2^254)
    report(i, count, first);
    return;
  }
  uint32_t any = 0;
  CQ_UNROLL for (int k = 0; k < 8; k++) any |= w[k];
  uint32_t o[8];
  if (any == 0 && ysign == 0) {  // the identity: (0, 0) in the raw layout
    CQ_UNROLL for (int k = 0; k < 8; k++) o[k] = 0;
    st8(&out[i].x, o);
    st8(&out[i].y, o);
    return;
  }
  const Fq29 xc = Fq29::unpack(w);  // canonical memory word: < q, normalised
  Fq29 r2, b, lit1 = Fq29::zero();
  CQ_UNROLL for (int k = 0; k < 9; k++) {
    r2.a[k] = SERDE_CONSTS.r2[k];  // < q, normalised
    b.a[k] = SERDE_CONSTS.b[k];    // 3 R' mod q: < q, normalised
  }
  lit1.a[0] = 1;
  const Fq29 x = Fq29::mul(xc, r2);        // 1 * 1 <= 128  ->  x R' < 2 q, normalised
  const Fq29 x2 = x.sqr();                 // 2 * 2 = 4 <= 121  ->  < 2 q
  const Fq29 x3 = Fq29::mul(x2, x);        // 2 * 2 = 4 <= 128  ->  < 2 q
  const Fq29 rhs = x3 + b;                 // limb-wise: < 3 q, limbs < 2^30
  const Fq29 y = sqrt_candidate29<FqP>(rhs);  // operand < 8 q with limbs < 2^30  ->  < 2 q, normalised
  if (!sqrt_is_root29<FqP>(y, rhs)) {         // y < 2 q normalised, rhs as above: x^3 + 3 is not a square
    report(i, count, first);
    return;
  }
  // the parity is that of the INTEGER y: a product with the literal 1 divides R' out.  (to_canonical_words() multiplies by the
  // field's one, R' mod q, and so returns the reduced representative of y R' -- still the Montgomery form.)
  const Fq29 yc = Fq29::mul(y, lit1);      // 2 * 1 <= 128  ->  y, < 2 q, normalised
  yc.pack(o);                              // < 2 q < 2^256
  Fq::cond_sub_p(o, 0);                    // canonical y
  Fq ym = y.to_mont256();                  // y < 2 q <= 64 q  ->  canonical R = 2^256 word
  if ((o[0] & 1u) != ysign) ym = ym.neg();
  const Fq xm = x.to_mont256();            // x < 2 q <= 64 q
  st8(&out[i].x, xm.v.l);
  st8(&out[i].y, ym.v.l);
}

// CurveAffine::to_bytes (derive/curve.rs:635-646)
__global__ void __launch_bounds__(256) g1_compress_kernel(const G1Affine* __restrict__ in, uint32_t n, uint8_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fq x, y;
  ld8(&in[i].x, x.v.l);
  ld8(&in[i].y, y.v.l);
  uint32_t o[8];
  if (x.is_zero() && y.is_zero()) {
    CQ_UNROLL for (int k = 0; k < 8; k++) o[k] = 0;
  } else {
    const U256 xc = x.to_canonical(), yc = y.to_canonical();
    CQ_UNROLL for (int k = 0; k < 8; k++) o[k] = xc.l[k];
    o[7] |= (yc.l[0] & 1u) << 31;
  }
  st8(out + (size_t)i * 32, o);
}

// `Fr::from_repr` (helpers.rs:68-79): canonical little-endian -> Montgomery words; values >= r are reported
__global__ void __launch_bounds__(256) fr_from_repr_kernel(const uint8_t* in, uint32_t n, Fr* out, uint32_t* __restrict__ count,
                                                           uint32_t* __restrict__ first) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  U256 w;
  ld8(in + (size_t)i * 32, w.l);
  if (!below_modulus<FrP>(w.l)) {
    report(i, count, first);
    return;
  }
  const Fr v = Fr::from_canonical(w);
  st8(out + i, v.v.l);
}

// `Fr::to_repr` (helpers.rs:81-91)
__global__ void __launch_bounds__(256) fr_to_repr_kernel(const Fr* in, uint32_t n, uint8_t* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fr v;
  ld8(in + i, v.v.l);
  const U256 w = v.to_canonical();
  st8(out + (size_t)i * 32, w.l);
}

// ---- G2 ---------------------------------------------------------------------------------------------------------------
// `GroupEncoding::from_bytes` for G2Affine (derive/curve.rs:603-627, compressed size 64; `Fq2::from_bytes`, fq2.rs:134-146):
// canonical x.c0 | x.c1 little-endian, bit 7 of byte 63 the parity of the canonical y.c0, 64 zero bytes the identity; no
// subgroup check.  One point per lane: about 670 dependent Fq products (sqrt2_29.hpp: 651; x to limb form and back 4, x^3 6,
// y to memory form 2).  Invalid: a component >= q, x^3 + b' not a square -- which covers x = 0 with the sign bit, b' being
// a non-square.  Reported indices are base + i: a caller converting an array in chunks gets indices in the whole array.
__global__ void __launch_bounds__(256) g2_decompress_kernel(const uint8_t* __restrict__ in, uint32_t n, uint32_t base, G2Affine* __restrict__ out,
                                                            uint32_t* __restrict__ count, uint32_t* __restrict__ first) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w0[8], w1[8];
  ld8(in + (size_t)i * 64, w0);
  ld8(in + (size_t)i * 64 + 32, w1);
  const uint32_t ysign = w1[7] >> 31;  // bit 7 of byte 63
  w1[7] &= 0x7fffffffu;
  if (!below_modulus<FqP>(w0) || !below_modulus<FqP>(w1)) {  // `Fq::from_bytes` fails on a non-canonical component
    report(base + i, count, first);
    return;
  }
  uint32_t any = 0;
  CQ_UNROLL for (int k = 0; k < 8; k++) any |= w0[k] | w1[k];
  uint32_t o[8];
  if (any == 0 && ysign == 0) {  // the identity: (0, 0, 0, 0) in the raw layout
    CQ_UNROLL for (int k = 0; k < 8; k++) o[k] = 0;
    st8(&out[i].x.c0, o);
    st8(&out[i].x.c1, o);
    st8(&out[i].y.c0, o);
    st8(&out[i].y.c1, o);
    return;
  }
  Fq29 r2;
  Fq2_29 b;
  CQ_UNROLL for (int k = 0; k < 9; k++) {
    r2.a[k] = SERDE_CONSTS.r2[k];     // < q, normalised
    b.c0.a[k] = SERDE2_CONSTS.b0[k];  // b' R' mod q per component: < q, normalised
    b.c1.a[k] = SERDE2_CONSTS.b1[k];
  }
  Fq2_29 x;
  x.c0 = Fq29::mul(Fq29::unpack(w0), r2);  // canonical memory word < q, normalised: 1 * 1 <= 128  ->  x.c0 R' < 2 q, normalised
  x.c1 = Fq29::mul(Fq29::unpack(w1), r2);
  // x leaves now (an invalid point's output is unspecified): nothing of it stays live across the two chains
  st8(&out[i].x.c0, x.c0.to_mont256().v.l);  // < 2 q <= 64 q
  st8(&out[i].x.c1, x.c1.to_mont256().v.l);
  const Fq2_29 x2 = x.sqr<2>();               // Ka = 2 <= 5  ->  < 2 q
  const Fq2_29 x3 = Fq2_29::mul<2>(x2, x);    // Ka Kb = 4 <= 64  ->  < 2 q
  const Fq2_29 rhs = x3 + b;                  // limb-wise: < 3 q per component, limbs < 2^30
  Fq2_29 y;
  if (!fq2_decoded_y29(rhs, ysign, y)) {      // operand < 8 q with limbs < 2^30: x^3 + b' is not a square
    report(base + i, count, first);
    return;
  }
  st8(&out[i].y.c0, y.c0.to_mont256().v.l);   // <= 2 q <= 64 q, normalised  ->  canonical R = 2^256 word
  st8(&out[i].y.c1, y.c1.to_mont256().v.l);
}

// `GroupEncoding::to_bytes` for G2Affine (derive/curve.rs:635-646; `Fq2::to_bytes`, fq2.rs:148-155)
__global__ void __launch_bounds__(256) g2_compress_kernel(const G2Affine* __restrict__ in, uint32_t n, uint8_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fq x0, x1, y0, y1;
  ld8(&in[i].x.c0, x0.v.l);
  ld8(&in[i].x.c1, x1.v.l);
  ld8(&in[i].y.c0, y0.v.l);
  ld8(&in[i].y.c1, y1.v.l);
  uint32_t o0[8], o1[8];
  if (x0.is_zero() && x1.is_zero() && y0.is_zero() && y1.is_zero()) {
    CQ_UNROLL for (int k = 0; k < 8; k++) o0[k] = o1[k] = 0;
  } else {
    const U256 c0 = x0.to_canonical(), c1 = x1.to_canonical(), yc = y0.to_canonical();
    CQ_UNROLL for (int k = 0; k < 8; k++) {
      o0[k] = c0.l[k];
      o1[k] = c1.l[k];
    }
    o1[7] |= (yc.l[0] & 1u) << 31;
  }
  st8(out + (size_t)i * 64, o0);
  st8(out + (size_t)i * 64 + 32, o1);
}

// SerdeFormat::RawBytes for G2Affine (`SerdeObject::from_raw_bytes`, derive/curve.rs:649-700): every coordinate below q and
// the point on the twist, or the identity.  `b` = 3 / (9 + i) in the memory form.
__global__ void __launch_bounds__(256) g2_validate_kernel(const G2Affine* __restrict__ pts, uint32_t n, uint32_t base, Fq2 b,
                                                          uint32_t* __restrict__ count, uint32_t* __restrict__ first) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fq2 x, y;
  ld8(&pts[i].x.c0, x.c0.v.l);
  ld8(&pts[i].x.c1, x.c1.v.l);
  ld8(&pts[i].y.c0, y.c0.v.l);
  ld8(&pts[i].y.c1, y.c1.v.l);
  bool ok = below_modulus<FqP>(x.c0.v.l) && below_modulus<FqP>(x.c1.v.l) && below_modulus<FqP>(y.c0.v.l) && below_modulus<FqP>(y.c1.v.l);
  if (ok && !(x.is_zero() && y.is_zero())) ok = y.sqr() == x.sqr() * x + b;
  if (!ok) report(base + i, count, first);
}

inline uint32_t blocks_for(uint32_t n) { return (n + 255) / 256; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

int serde_verdict_reset(cq_ctx* c, uint32_t* count_dev, uint32_t* first_dev, size_t cells) {
  CQ_HIP(c, hipMemsetAsync(count_dev, 0, cells * sizeof(uint32_t), c->stream));
  CQ_HIP(c, hipMemsetAsync(first_dev, 0xff, cells * sizeof(uint32_t), c->stream));
  return CQ_OK;
}

int g1_decompress(cq_ctx* c, const uint8_t* in, uint32_t n, G1Affine* out, uint32_t* count_dev, uint32_t* first_dev) {
  if (!n) return CQ_OK;
  if (!aligned16(in) || !aligned16(out)) return c->fail(CQ_ERR_ARG, "g1_decompress: buffers must be 16-byte aligned");
  hipEvent_t pe = c->prof_begin(CQ_PROF_G1_DECOMPRESS);
  g1_decompress_kernel<<<blocks_for(n), 256, 0, c->stream>>>(in, n, out, count_dev, first_dev);
  c->prof_end(pe);
  return hipGetLastError() == hipSuccess ? CQ_OK : c->fail(CQ_ERR_HIP, "g1_decompress launch failed");
}

int g1_compress(cq_ctx* c, const G1Affine* in, uint32_t n, uint8_t* out) {
  if (!n) return CQ_OK;
  if (!aligned16(in) || !aligned16(out)) return c->fail(CQ_ERR_ARG, "g1_compress: buffers must be 16-byte aligned");
  g1_compress_kernel<<<blocks_for(n), 256, 0, c->stream>>>(in, n, out);
  return hipGetLastError() == hipSuccess ? CQ_OK : c->fail(CQ_ERR_HIP, "g1_compress launch failed");
}

int fr_from_repr(cq_ctx* c, const uint8_t* in, uint32_t n, Fr* out, uint32_t* count_dev, uint32_t* first_dev) {
  if (!n) return CQ_OK;
  if (!aligned16(in) || !aligned16(out)) return c->fail(CQ_ERR_ARG, "fr_from_repr: buffers must be 16-byte aligned");
  fr_from_repr_kernel<<<blocks_for(n), 256, 0, c->stream>>>(in, n, out, count_dev, first_dev);
  return hipGetLastError() == hipSuccess ? CQ_OK : c->fail(CQ_ERR_HIP, "fr_from_repr launch failed");
}

int fr_to_repr(cq_ctx* c, const Fr* in, uint32_t n, uint8_t* out) {
  if (!n) return CQ_OK;
  if (!aligned16(in) || !aligned16(out)) return c->fail(CQ_ERR_ARG, "fr_to_repr: buffers must be 16-byte aligned");
  fr_to_repr_kernel<<<blocks_for(n), 256, 0, c->stream>>>(in, n, out);
  return hipGetLastError() == hipSuccess ? CQ_OK : c->fail(CQ_ERR_HIP, "fr_to_repr launch failed");
}

int g2_decompress(cq_ctx* c, const uint8_t* in, uint32_t n, uint32_t base, G2Affine* out, uint32_t* count_dev, uint32_t* first_dev) {
  if (!n) return CQ_OK;
  if (!aligned16(in) || !aligned16(out)) return c->fail(CQ_ERR_ARG, "g2_decompress: buffers must be 16-byte aligned");
  hipEvent_t pe = c->prof_begin(CQ_PROF_G2_DECOMPRESS);
  g2_decompress_kernel<<<blocks_for(n), 256, 0, c->stream>>>(in, n, base, out, count_dev, first_dev);
  c->prof_end(pe);
  return hipGetLastError() == hipSuccess ? CQ_OK : c->fail(CQ_ERR_HIP, "g2_decompress launch failed");
}

int g2_compress(cq_ctx* c, const G2Affine* in, uint32_t n, uint8_t* out) {
  if (!n) return CQ_OK;
  if (!aligned16(in) || !aligned16(out)) return c->fail(CQ_ERR_ARG, "g2_compress: buffers must be 16-byte aligned");
  g2_compress_kernel<<<blocks_for(n), 256, 0, c->stream>>>(in, n, out);
  return hipGetLastError() == hipSuccess ? CQ_OK : c->fail(CQ_ERR_HIP, "g2_compress launch failed");
}

int g2_validate(cq_ctx* c, const G2Affine* pts, uint32_t n, uint32_t base, uint32_t* count_dev, uint32_t* first_dev) {
  if (!n) return CQ_OK;
  if (!aligned16(pts)) return c->fail(CQ_ERR_ARG, "g2_validate: buffer must be 16-byte aligned");
  g2_validate_kernel<<<blocks_for(n), 256, 0, c->stream>>>(pts, n, base, g2_b(), count_dev, first_dev);
  return hipGetLastError() == hipSuccess ? CQ_OK : c->fail(CQ_ERR_HIP, "g2_validate launch failed");
}

}  // namespace cq

using namespace cq;

namespace {
// Runs one checking conversion with its verdict words in the entry scratch, waits, and turns a verdict into CQ_ERR_ARG
template <class Launch>
int checked_conversion(cq_ctx* c, const char* what, size_t* first_bad, Launch&& launch) {
  void* cell;
  int rc;
  if ((rc = c->ensure_scratch(Scratch::EntryA, 64, &cell)) != CQ_OK) return rc;
  uint32_t* count_dev = (uint32_t*)cell;
  uint32_t* first_dev = count_dev + 1;
  if ((rc = serde_verdict_reset(c, count_dev, first_dev, 1)) != CQ_OK) return rc;
  if ((rc = launch(count_dev, first_dev)) != CQ_OK) return rc;
  uint32_t verdict[2] = {0, 0};
  CQ_HIP(c, hipMemcpyAsync(verdict, cell, sizeof(verdict), hipMemcpyDeviceToHost, c->stream));
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  if (verdict[0]) {
    if (first_bad) *first_bad = verdict[1];
    return c->fail(CQ_ERR_ARG, std::string(what) + ": invalid encoding at index " + std::to_string(verdict[1]) + " (" +
                                   std::to_string(verdict[0]) + " invalid in all)");
  }
  return CQ_OK;
}
}  // namespace

extern "C" {

int cq_g1_decompress_dev(cq_ctx* c, const uint8_t* bytes_dev, size_t n, uint64_t* out_affine_dev, size_t* first_bad) {
  if (!c || (n && (!bytes_dev || !out_affine_dev)) || n > 0x7fffffffull) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  return checked_conversion(c, "g1 decompress", first_bad, [&](uint32_t* count_dev, uint32_t* first_dev) {
    return g1_decompress(c, bytes_dev, (uint32_t)n, (G1Affine*)out_affine_dev, count_dev, first_dev);
  });
}

int cq_g1_compress_dev(cq_ctx* c, const uint64_t* affine_dev, size_t n, uint8_t* bytes_dev) {
  if (!c || (n && (!affine_dev || !bytes_dev)) || n > 0x7fffffffull) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  return g1_compress(c, (const G1Affine*)affine_dev, (uint32_t)n, bytes_dev);
}

int cq_g2_decompress_dev(cq_ctx* c, const uint8_t* bytes_dev, size_t n, uint64_t* out_affine_dev, size_t* first_bad) {
  if (!c || (n && (!bytes_dev || !out_affine_dev)) || n > 0x7fffffffull) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  return checked_conversion(c, "g2 decompress", first_bad, [&](uint32_t* count_dev, uint32_t* first_dev) {
    return g2_decompress(c, bytes_dev, (uint32_t)n, 0, (G2Affine*)out_affine_dev, count_dev, first_dev);
  });
}

int cq_g2_compress_dev(cq_ctx* c, const uint64_t* affine_dev, size_t n, uint8_t* bytes_dev) {
  if (!c || (n && (!affine_dev || !bytes_dev)) || n > 0x7fffffffull) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  return g2_compress(c, (const G2Affine*)affine_dev, (uint32_t)n, bytes_dev);
}

int cq_fr_from_repr_dev(cq_ctx* c, const uint8_t* bytes_dev, size_t n, uint64_t* out_dev, size_t* first_bad) {
  if (!c || (n && (!bytes_dev || !out_dev)) || n > 0x7fffffffull) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  return checked_conversion(c, "fr from_repr", first_bad, [&](uint32_t* count_dev, uint32_t* first_dev) {
    return fr_from_repr(c, bytes_dev, (uint32_t)n, (Fr*)out_dev, count_dev, first_dev);
  });
}

int cq_fr_to_repr_dev(cq_ctx* c, const uint64_t* in_dev, size_t n, uint8_t* bytes_dev) {
  if (!c || (n && (!in_dev || !bytes_dev)) || n > 0x7fffffffull) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  return fr_to_repr(c, (const Fr*)in_dev, (uint32_t)n, bytes_dev);
}

}  // extern "C"

// SerdeFormat::Processed on the device: point decompression / compression (derive/curve.rs:603-646) and the canonical
// scalar encodings (helpers.rs:68-91), with their C entry points.  The params and proving-key readers built on them live
// next to their raw twins (capi_msm.hip, capi_cq.hip).
#include <cstdint>
#include <string>
#include "ctx.hpp"
#include "serde.hpp"
#include "sqrt29.hpp"

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

// C ABI: best_multiexp and ParamsKZG::commit / commit_lagrange.  See include/cq_halo2.h.  (The engine behind the entry
// points -- launch planner, table registry -- is msm_multi.hip.)
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "ctx.hpp"
#include "msm.hpp"
#include "g1fft.hpp"
#include "setup.hpp"
#include "cq.hpp"
#include "serde.hpp"
#include "msm_g2.hpp"

using namespace cq;

static int msm_batch(cq_ctx* c, const Fr* const* scalars, const G1Affine* bases, size_t len, size_t count,
                     uint64_t* out_jac) {
  std::vector<const G1Affine*> bp(count, bases);
  return cq_msm_multi(c, scalars, bp.data(), len, count, out_jac);
}

namespace {
// destroys a half-built cq_params on every failing return (CQ_HIP included); release() on success
struct ParamsGuard {
  cq_params* p;
  explicit ParamsGuard(cq_params* p_) : p(p_) {}
  ~ParamsGuard() {
    if (p) cq_params_destroy(p);
  }
  cq_params* release() {
    cq_params* q = p;
    p = nullptr;
    return q;
  }
};
cq_params* params_new(cq_ctx* c, uint32_t k) {
  cq_params* p = new cq_params();
  p->ctx = c;
  p->k = k;
  p->n = (size_t)1 << k;
  p->g = nullptr;
  p->g_lagrange = nullptr;
  return p;
}
}  // namespace

extern "C" {

int cq_msm_precompute_dev(cq_ctx* c, const uint64_t* bases_dev, size_t n) {
  if (!c || !bases_dev) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  return msm_register_tables(c, (const G1Affine*)bases_dev, n);
}

int cq_msm_forget_dev(cq_ctx* c, const uint64_t* bases_dev) {
  if (!c || !bases_dev) return CQ_ERR_ARG;
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  msm_unregister_tables(c, bases_dev);
  return CQ_OK;
}

int cq_msm_set_precompute(cq_ctx* c, int on) {
  if (!c) return CQ_ERR_ARG;
  c->msm_precompute = on != 0;
  return CQ_OK;
}

int cq_msm_set_table_window(cq_ctx* c, uint32_t bits) {
  if (!c || (bits != 0 && (bits < MSM_TABLE_C_MIN || bits > MSM_TABLE_C_MAX))) return CQ_ERR_ARG;
  c->msm_table_c = bits;
  return CQ_OK;
}

int cq_msm_table_width_dev(cq_ctx* c, const uint64_t* bases_dev, size_t n, uint32_t preferred_bits, uint32_t* bits) {
  if (!c || !bases_dev || !bits) return CQ_ERR_ARG;
  const cq_ctx::MsmTable* t = c->find_msm_table(bases_dev, n, nullptr, preferred_bits);
  *bits = t ? t->c : 0;
  return CQ_OK;
}

int cq_msm_bucket_sums_dev(cq_ctx* c, const uint64_t* const* bases_dev, size_t arrays, int packed, const uint32_t* index_dev, size_t n,
                           size_t buckets, uint64_t* out_dev) {
  if (!c || !bases_dev || !index_dev || !out_dev || !arrays || arrays > MSM_MAX_BATCH || !n || n > ((size_t)1 << 26) || !buckets ||
      buckets > ((size_t)1 << (MSM_TABLE_C - 1)))
    return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  void* conv = nullptr;
  int rc;
  if (!packed && (rc = c->ensure_scratch(Scratch::EntryB, arrays * n * sizeof(G1Affine), &conv)) != CQ_OK) return rc;
  std::vector<const uint32_t*> idx(arrays, index_dev);
  std::vector<const G1Affine*> bs(arrays);
  for (size_t a = 0; a < arrays; a++) {
    if (!bases_dev[a]) return CQ_ERR_ARG;
    bs[a] = (const G1Affine*)bases_dev[a];
    if (!packed) {
      G1Affine* dst = (G1Affine*)conv + a * n;
      if (msm_bases29(c, bs[a], (uint32_t)n, dst) != 0) return c->fail(CQ_ERR_HIP, "bucket sums: bases");
      bs[a] = dst;
    }
  }
  if (msm_bucket_sums(c, idx.data(), bs.data(), (uint32_t)n, (uint32_t)arrays, (uint32_t)buckets, (G1Affine*)out_dev) != 0)
    return c->fail(CQ_ERR_HIP, "bucket-sum launch failed");
  return c->wait(c->stream);
}

int cq_msm_set_window(cq_ctx* c, uint32_t bits) {
  if (!c || (bits != 0 && (bits < 2 || bits > 15))) return CQ_ERR_ARG;
  c->msm_c = bits;
  return CQ_OK;
}

int cq_best_multiexp_dev(cq_ctx* c, const uint64_t* coeffs_dev, const uint64_t* bases_dev, size_t len,
                         uint64_t out_jac[12]) {
  if (!c || !out_jac || (len && (!coeffs_dev || !bases_dev))) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  const Fr* sc = (const Fr*)coeffs_dev;
  return msm_batch(c, &sc, (const G1Affine*)bases_dev, len, 1, out_jac);
}

int cq_msm_batch_dev(cq_ctx* c, const uint64_t* const* coeffs_dev, const uint64_t* bases_dev, size_t len,
                     size_t count, uint64_t* out_jac) {
  if (!c || !out_jac || !coeffs_dev || (len && !bases_dev)) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  return msm_batch(c, (const Fr* const*)coeffs_dev, (const G1Affine*)bases_dev, len, count, out_jac);
}

int cq_best_multiexp(cq_ctx* c, const uint64_t* coeffs, const uint64_t* bases, size_t len, uint64_t out_jac[12]) {
  if (!c || !out_jac || (len && (!coeffs || !bases))) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  if (len == 0) {
    memset(out_jac, 0, 12 * sizeof(uint64_t));
    return CQ_OK;
  }
  void *ds, *db;
  int rc;
  if ((rc = c->ensure_scratch(Scratch::EntryA, len * sizeof(Fr), &ds)) != CQ_OK) return rc;
  if ((rc = c->ensure_scratch(Scratch::EntryB, len * sizeof(G1Affine), &db)) != CQ_OK) return rc;
  CQ_HIP(c, hipMemcpyAsync(ds, coeffs, len * sizeof(Fr), hipMemcpyHostToDevice, c->stream));
  CQ_HIP(c, hipMemcpyAsync(db, bases, len * sizeof(G1Affine), hipMemcpyHostToDevice, c->stream));
  const Fr* sc = (const Fr*)ds;
  return msm_batch(c, &sc, (const G1Affine*)db, len, 1, out_jac);
}

// ---- ParamsKZG ---------------------------------------------------------------------------------
int cq_params_create(cq_ctx* c, uint32_t k, const uint64_t* g, const uint64_t* g_lagrange, cq_params** out) {
  if (!c || !g || !g_lagrange || !out || k > FR_S) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  *out = nullptr;
  cq_params* p = params_new(c, k);
  ParamsGuard guard(p);
  const size_t bytes = p->n * sizeof(G1Affine);
  hipError_t e;
  if ((e = hipMalloc(&p->g, bytes)) != hipSuccess || (e = hipMalloc(&p->g_lagrange, bytes)) != hipSuccess)
    return c->hip_fail(e, "hipMalloc(params)");
  CQ_HIP(c, hipMemcpyAsync(p->g, g, bytes, hipMemcpyHostToDevice, c->stream));
  CQ_HIP(c, hipMemcpyAsync(p->g_lagrange, g_lagrange, bytes, hipMemcpyHostToDevice, c->stream));
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  if (c->msm_precompute) {
    int rc2;
    if ((rc2 = msm_register_tables(c, p->g, p->n)) != CQ_OK) return rc2;
    if ((rc2 = msm_register_tables(c, p->g_lagrange, p->n)) != CQ_OK) return rc2;
  }
  *out = guard.release();
  return CQ_OK;
}

/* ParamsKZG from g alone: g_lagrange = g_to_lagrange(g, k) (arithmetic.rs:277-301) straight into the resident array */
int cq_params_from_powers(cq_ctx* c, uint32_t k, const uint64_t* g, int g_on_device, cq_params** out) {
  if (!c || !g || !out || k > FR_S) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  *out = nullptr;
  cq_params* p = params_new(c, k);
  ParamsGuard guard(p);
  const size_t bytes = p->n * sizeof(G1Affine);
  hipError_t e;
  if ((e = hipMalloc(&p->g, bytes)) != hipSuccess || (e = hipMalloc(&p->g_lagrange, bytes)) != hipSuccess)
    return c->hip_fail(e, "hipMalloc(params)");
  CQ_HIP(c, hipMemcpyAsync(p->g, g, bytes, g_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
  int rc;
  if ((rc = g1_to_lagrange(c, p->g, k, p->g_lagrange, true)) != CQ_OK) return rc;  // waits for the stream
  if (c->msm_precompute) {
    if ((rc = msm_register_tables(c, p->g, p->n)) != CQ_OK) return rc;
    if ((rc = msm_register_tables(c, p->g_lagrange, p->n)) != CQ_OK) return rc;
  }
  *out = guard.release();
  return CQ_OK;
}

/* ParamsKZG::setup_from_toxic_waste (kzg/commitment.rs:209-276), computed on the GPU */
int cq_params_setup_from_toxic_waste(cq_ctx* c, uint32_t k, const uint64_t s[4], cq_params** out) {
  if (!c || !s || !out || k > FR_S) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  *out = nullptr;
  cq_params* p = params_new(c, k);
  ParamsGuard guard(p);
  const size_t bytes = p->n * sizeof(G1Affine);
  hipError_t e;
  if ((e = hipMalloc(&p->g, bytes)) != hipSuccess || (e = hipMalloc(&p->g_lagrange, bytes)) != hipSuccess)
    return c->hip_fail(e, "hipMalloc(params)");
  void* tmp;
  int rc;
  if ((rc = c->ensure_scratch(Scratch::EntryA, p->n * sizeof(Fr), &tmp)) != CQ_OK) return rc;
  rc = srs_powers_and_lagrange(c, k, Fr::from_limbs64(s), p->g, p->g_lagrange, (Fr*)tmp, nullptr);
  if (rc != CQ_OK) return rc;
  if (c->msm_precompute) {
    if ((rc = msm_register_tables(c, p->g, p->n)) != CQ_OK) return rc;
    if ((rc = msm_register_tables(c, p->g_lagrange, p->n)) != CQ_OK) return rc;
  }
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  // g2 = generator, s_g2 = [s]_2 (commitment.rs:265-266): the first two G2 powers
  void* two;
  if ((rc = c->ensure_scratch(Scratch::EntryB, 2 * sizeof(G2Affine), &two)) != CQ_OK) return rc;
  if ((rc = g2_srs_powers(c, Fr::from_limbs64(s), 2, (G2Affine*)two)) != CQ_OK) return rc;
  uint64_t tail[32];
  CQ_HIP(c, hipMemcpyAsync(tail, two, sizeof(tail), hipMemcpyDeviceToHost, c->stream));
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  memcpy(p->g2, tail, sizeof(p->g2));
  memcpy(p->s_g2, tail + 16, sizeof(p->s_g2));
  p->has_g2 = true;
  *out = guard.release();
  return CQ_OK;
}

/* scalars[i] * G for device-resident scalars (every SRS element has this form) */
int cq_fixed_base_mul_dev(cq_ctx* c, const uint64_t* scalars_dev, size_t n, uint64_t* out_affine_dev) {
  if (!c || (n && (!scalars_dev || !out_affine_dev)) || n > 0x7fffffffull) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  return fixed_base_mul(c, (const Fr*)scalars_dev, (uint32_t)n, (G1Affine*)out_affine_dev);
}

/* ParamsKZG::read_custom with RawBytes / RawBytesUnchecked (kzg/commitment.rs:383-459):
 * k:u32 LE | n x 64 B g | n x 64 B g_lagrange | [128 B g2 | 128 B s_g2, ignored here: cq_params_read_full] -- straight into HBM */
int cq_params_read_raw(cq_ctx* c, const uint8_t* buf, size_t len, int checked, cq_params** out) {
  if (!c || !buf || !out || len < 4) return CQ_ERR_ARG;
  uint32_t k;
  memcpy(&k, buf, 4);
  if (k > FR_S) return c->fail(CQ_ERR_ARG, "params: k out of range");
  const size_t n = (size_t)1 << k;
  if (len < 4 + 2 * n * sizeof(G1Affine)) return c->fail(CQ_ERR_ARG, "params: buffer too short");
  CQ_HIP(c, hipSetDevice(c->device));
  *out = nullptr;
  cq_params* p = params_new(c, k);
  ParamsGuard guard(p);
  const size_t bytes = n * sizeof(G1Affine);
  if (hipMalloc(&p->g, bytes) != hipSuccess || hipMalloc(&p->g_lagrange, bytes) != hipSuccess)
    return c->fail(CQ_ERR_HIP, "hipMalloc(params)");
  CQ_HIP(c, hipMemcpyAsync(p->g, buf + 4, bytes, hipMemcpyHostToDevice, c->stream));
  CQ_HIP(c, hipMemcpyAsync(p->g_lagrange, buf + 4 + bytes, bytes, hipMemcpyHostToDevice, c->stream));
  if (checked) {  // SerdeFormat::RawBytes: coordinates < q and on the curve
    void* tmp;
    int rc;
    if ((rc = c->ensure_scratch(Scratch::EntryA, 64, &tmp)) != CQ_OK) return rc;
    CQ_HIP(c, hipMemsetAsync(tmp, 0, 4, c->stream));
    if ((rc = g1_validate(c, p->g, (uint32_t)n, (uint32_t*)tmp)) != CQ_OK) return rc;
    if ((rc = g1_validate(c, p->g_lagrange, (uint32_t)n, (uint32_t*)tmp)) != CQ_OK) return rc;
    uint32_t bad = 0;
    CQ_HIP(c, hipMemcpyAsync(&bad, tmp, 4, hipMemcpyDeviceToHost, c->stream));
    CQ_HIP(c, hipStreamSynchronize(c->stream));
    if (bad) return c->fail(CQ_ERR_ARG, "params: invalid point encoding");
  }
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  if (c->msm_precompute) {
    int rc2;
    if ((rc2 = msm_register_tables(c, p->g, p->n)) != CQ_OK) return rc2;
    if ((rc2 = msm_register_tables(c, p->g_lagrange, p->n)) != CQ_OK) return rc2;
  }
  *out = guard.release();
  return CQ_OK;
}

/* ParamsKZG::read_custom with SerdeFormat::Processed (kzg/commitment.rs:383-459):
 * k:u32 LE | n x 32 B g | n x 32 B g_lagrange | [2 x 64 B compressed g2, s_g2: ignored here, cq_params_read_full] -- the compressed bytes are staged
 * in the entry scratch and decompressed straight into the resident arrays */
static int params_read_processed(cq_ctx* c, const uint8_t* buf, size_t len, cq_params** out) {
  if (!c || !buf || !out || len < 4) return CQ_ERR_ARG;
  uint32_t k;
  memcpy(&k, buf, 4);
  if (k > FR_S) return c->fail(CQ_ERR_ARG, "params: k out of range");
  const size_t n = (size_t)1 << k, half = n * 32;
  if (len < 4 + 2 * half) return c->fail(CQ_ERR_ARG, "params: buffer too short");
  CQ_HIP(c, hipSetDevice(c->device));
  *out = nullptr;
  cq_params* p = params_new(c, k);
  ParamsGuard guard(p);
  if (hipMalloc(&p->g, n * sizeof(G1Affine)) != hipSuccess || hipMalloc(&p->g_lagrange, n * sizeof(G1Affine)) != hipSuccess)
    return c->fail(CQ_ERR_HIP, "hipMalloc(params)");
  void *stage, *cells;
  int rc;
  if ((rc = c->ensure_scratch(Scratch::EntryB, 2 * half, &stage)) != CQ_OK) return rc;
  if ((rc = c->ensure_scratch(Scratch::EntryA, 64, &cells)) != CQ_OK) return rc;
  uint32_t* count_dev = (uint32_t*)cells;  // [0], [1]: g, g_lagrange
  uint32_t* first_dev = count_dev + 2;
  if ((rc = serde_verdict_reset(c, count_dev, first_dev, 2)) != CQ_OK) return rc;
  CQ_HIP(c, hipMemcpyAsync(stage, buf + 4, 2 * half, hipMemcpyHostToDevice, c->stream));
  if ((rc = g1_decompress(c, (const uint8_t*)stage, (uint32_t)n, p->g, count_dev, first_dev)) != CQ_OK) return rc;
  if ((rc = g1_decompress(c, (const uint8_t*)stage + half, (uint32_t)n, p->g_lagrange, count_dev + 1, first_dev + 1)) != CQ_OK) return rc;
  uint32_t verdict[4] = {0, 0, 0, 0};
  CQ_HIP(c, hipMemcpyAsync(verdict, cells, sizeof(verdict), hipMemcpyDeviceToHost, c->stream));
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  for (int a = 0; a < 2; a++)
    if (verdict[a])
      return c->fail(CQ_ERR_ARG, std::string("params: invalid point encoding at ") + (a ? "g_lagrange[" : "g[") + std::to_string(verdict[2 + a]) +
                                     "] (" + std::to_string(verdict[a]) + " invalid in that array)");
  if (c->msm_precompute) {
    if ((rc = msm_register_tables(c, p->g, p->n)) != CQ_OK) return rc;
    if ((rc = msm_register_tables(c, p->g_lagrange, p->n)) != CQ_OK) return rc;
  }
  *out = guard.release();
  return CQ_OK;
}

int cq_params_read(cq_ctx* c, const uint8_t* buf, size_t len, int format, cq_params** out) {
  switch (format) {
    case CQ_SERDE_PROCESSED: return params_read_processed(c, buf, len, out);
    case CQ_SERDE_RAW_BYTES: return cq_params_read_raw(c, buf, len, 1, out);
    case CQ_SERDE_RAW_BYTES_UNCHECKED: return cq_params_read_raw(c, buf, len, 0, out);
  }
  return c ? c->fail(CQ_ERR_ARG, "params: unknown serde format") : CQ_ERR_ARG;
}

size_t cq_params_serialized_size(const cq_params* p, int format) {
  if (!p) return 0;
  if (format == CQ_SERDE_PROCESSED) return 4 + 2 * p->n * 32;
  if (format == CQ_SERDE_RAW_BYTES || format == CQ_SERDE_RAW_BYTES_UNCHECKED) return 4 + 2 * p->n * sizeof(G1Affine);
  return 0;
}

/* G1 part of ParamsKZG::write_custom (commitment.rs:366-379); Processed: points compressed on the GPU into the entry scratch */
int cq_params_write(cq_params* p, int format, uint8_t* buf, size_t cap, size_t* written) {
  if (!p || !buf || !written) return CQ_ERR_ARG;
  cq_ctx* c = p->ctx;
  if (format == CQ_SERDE_RAW_BYTES || format == CQ_SERDE_RAW_BYTES_UNCHECKED) return cq_params_write_raw(p, buf, cap, written);
  if (format != CQ_SERDE_PROCESSED) return c->fail(CQ_ERR_ARG, "params: unknown serde format");
  const size_t half = p->n * 32;
  if (cap < 4 + 2 * half) return c->fail(CQ_ERR_ARG, "params: output buffer too small");
  CQ_HIP(c, hipSetDevice(c->device));
  void* stage;
  int rc;
  if ((rc = c->ensure_scratch(Scratch::EntryB, 2 * half, &stage)) != CQ_OK) return rc;
  if ((rc = g1_compress(c, p->g, (uint32_t)p->n, (uint8_t*)stage)) != CQ_OK) return rc;
  if ((rc = g1_compress(c, p->g_lagrange, (uint32_t)p->n, (uint8_t*)stage + half)) != CQ_OK) return rc;
  memcpy(buf, &p->k, 4);
  CQ_HIP(c, hipMemcpyAsync(buf + 4, stage, 2 * half, hipMemcpyDeviceToHost, c->stream));
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  *written = 4 + 2 * half;
  return CQ_OK;
}

// ---- g2 / s_g2 and the complete ParamsKZG stream ------------------------------------------------------------------------
int cq_params_set_g2(cq_params* p, const uint64_t g2[16], const uint64_t s_g2[16]) {
  if (!p || !g2 || !s_g2) return CQ_ERR_ARG;
  memcpy(p->g2, g2, sizeof(p->g2));
  memcpy(p->s_g2, s_g2, sizeof(p->s_g2));
  p->has_g2 = true;
  return CQ_OK;
}

int cq_params_g2(const cq_params* p, uint64_t g2[16], uint64_t s_g2[16]) {
  if (!p || !g2 || !s_g2) return CQ_ERR_ARG;
  if (!p->has_g2) return p->ctx->fail(CQ_ERR_ARG, "params: no g2 / s_g2 held (read_full, set_g2 or setup_from_toxic_waste provide them)");
  memcpy(g2, p->g2, sizeof(p->g2));
  memcpy(s_g2, p->s_g2, sizeof(p->s_g2));
  return CQ_OK;
}

static size_t g2_point_size(int format) {
  if (format == CQ_SERDE_PROCESSED) return 64;
  if (format == CQ_SERDE_RAW_BYTES || format == CQ_SERDE_RAW_BYTES_UNCHECKED) return sizeof(G2Affine);
  return 0;
}

size_t cq_params_serialized_size_full(const cq_params* p, int format) {
  const size_t g1 = cq_params_serialized_size(p, format);
  return g1 ? g1 + 2 * g2_point_size(format) : 0;
}

/* ParamsKZG::read_custom (commitment.rs:383-459), tail included: the G1 part by cq_params_read, then g2 | s_g2 staged in the
 * entry scratch and decompressed / validated by the G2 kernels of serde.hip */
int cq_params_read_full(cq_ctx* c, const uint8_t* buf, size_t len, int format, cq_params** out) {
  if (!c || !buf || !out || len < 4) return CQ_ERR_ARG;
  const size_t psz = g2_point_size(format);
  if (!psz) return c->fail(CQ_ERR_ARG, "params: unknown serde format");
  uint32_t k;
  memcpy(&k, buf, 4);
  if (k > FR_S) return c->fail(CQ_ERR_ARG, "params: k out of range");
  const size_t g1 = 4 + 2 * ((size_t)1 << k) * (psz / 2);
  if (len < g1 + 2 * psz) return c->fail(CQ_ERR_ARG, "params: buffer too short for the full stream (g2 | s_g2 missing)");
  *out = nullptr;
  cq_params* p = nullptr;
  int rc = cq_params_read(c, buf, len, format, &p);
  if (rc != CQ_OK) return rc;
  ParamsGuard guard(p);
  const uint8_t* tail = buf + g1;
  if (format == CQ_SERDE_RAW_BYTES_UNCHECKED) {
    memcpy(p->g2, tail, sizeof(p->g2));
    memcpy(p->s_g2, tail + sizeof(G2Affine), sizeof(p->s_g2));
  } else {
    void *stage, *cells;
    if ((rc = c->ensure_scratch(Scratch::EntryB, 2 * 64 + 2 * sizeof(G2Affine), &stage)) != CQ_OK) return rc;
    if ((rc = c->ensure_scratch(Scratch::EntryA, 64, &cells)) != CQ_OK) return rc;
    uint32_t* count_dev = (uint32_t*)cells;
    uint32_t* first_dev = count_dev + 1;
    G2Affine* pts = (G2Affine*)((uint8_t*)stage + 2 * 64);
    if ((rc = serde_verdict_reset(c, count_dev, first_dev, 1)) != CQ_OK) return rc;
    if (format == CQ_SERDE_PROCESSED) {
      CQ_HIP(c, hipMemcpyAsync(stage, tail, 2 * 64, hipMemcpyHostToDevice, c->stream));
      if ((rc = g2_decompress(c, (const uint8_t*)stage, 2, 0, pts, count_dev, first_dev)) != CQ_OK) return rc;
    } else {
      CQ_HIP(c, hipMemcpyAsync(pts, tail, 2 * sizeof(G2Affine), hipMemcpyHostToDevice, c->stream));
      if ((rc = g2_validate(c, pts, 2, 0, count_dev, first_dev)) != CQ_OK) return rc;
    }
    uint32_t verdict[2] = {0, 0};
    uint64_t both[32];
    CQ_HIP(c, hipMemcpyAsync(verdict, cells, sizeof(verdict), hipMemcpyDeviceToHost, c->stream));
    CQ_HIP(c, hipMemcpyAsync(both, pts, sizeof(both), hipMemcpyDeviceToHost, c->stream));
    CQ_HIP(c, hipStreamSynchronize(c->stream));
    if (verdict[0])
      return c->fail(CQ_ERR_ARG, std::string("params: invalid point encoding at ") + (verdict[1] ? "s_g2" : "g2") + " (" +
                                     std::to_string(verdict[0]) + " of the two G2 points invalid)");
    memcpy(p->g2, both, sizeof(p->g2));
    memcpy(p->s_g2, both + 16, sizeof(p->s_g2));
  }
  p->has_g2 = true;
  *out = guard.release();
  return CQ_OK;
}

/* ParamsKZG::write_custom (commitment.rs:366-379), tail included */
int cq_params_write_full(cq_params* p, int format, uint8_t* buf, size_t cap, size_t* written) {
  if (!p || !buf || !written) return CQ_ERR_ARG;
  cq_ctx* c = p->ctx;
  const size_t psz = g2_point_size(format);
  if (!psz) return c->fail(CQ_ERR_ARG, "params: unknown serde format");
  if (!p->has_g2) return c->fail(CQ_ERR_ARG, "params: no g2 / s_g2 held, the full stream cannot be written");
  const size_t g1 = cq_params_serialized_size(p, format);
  if (cap < g1 + 2 * psz) return c->fail(CQ_ERR_ARG, "params: output buffer too small");
  size_t w = 0;
  int rc = cq_params_write(p, format, buf, cap, &w);
  if (rc != CQ_OK) return rc;
  if (format == CQ_SERDE_PROCESSED) {
    void* stage;
    if ((rc = c->ensure_scratch(Scratch::EntryB, 2 * 64 + 2 * sizeof(G2Affine), &stage)) != CQ_OK) return rc;
    G2Affine* pts = (G2Affine*)((uint8_t*)stage + 2 * 64);
    CQ_HIP(c, hipMemcpyAsync(pts, p->g2, sizeof(p->g2), hipMemcpyHostToDevice, c->stream));
    CQ_HIP(c, hipMemcpyAsync(pts + 1, p->s_g2, sizeof(p->s_g2), hipMemcpyHostToDevice, c->stream));
    if ((rc = g2_compress(c, pts, 2, (uint8_t*)stage)) != CQ_OK) return rc;
    CQ_HIP(c, hipMemcpyAsync(buf + w, stage, 2 * 64, hipMemcpyDeviceToHost, c->stream));
    CQ_HIP(c, hipStreamSynchronize(c->stream));
  } else {
    memcpy(buf + w, p->g2, sizeof(p->g2));
    memcpy(buf + w + sizeof(G2Affine), p->s_g2, sizeof(p->s_g2));
  }
  *written = w + 2 * psz;
  return CQ_OK;
}

int cq_g_to_lagrange_dev(cq_ctx* c, const uint64_t* g_dev, uint32_t k, uint64_t* g_lagrange_dev) {
  if (!c || !g_dev || !g_lagrange_dev || k > 26) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  return g1_to_lagrange(c, (const G1Affine*)g_dev, k, (G1Affine*)g_lagrange_dev);
}

// ParamsKZG::downsize (kzg/commitment.rs:480-492)
int cq_g_to_lagrange_windowed_dev(cq_ctx* c, const uint64_t* g_dev, uint32_t k, uint64_t* g_lagrange_dev) {
  if (!c || !g_dev || !g_lagrange_dev || k > FR_S) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  return g1_to_lagrange(c, (const G1Affine*)g_dev, k, (G1Affine*)g_lagrange_dev, true);
}

int cq_params_downsize(cq_params* p, uint32_t k, cq_params** out) {
  if (!p || !out || k > p->k) return CQ_ERR_ARG;  // `assert!(k <= self.k)`
  cq_ctx* c = p->ctx;
  CQ_HIP(c, hipSetDevice(c->device));
  *out = nullptr;
  cq_params* q = params_new(c, k);
  ParamsGuard guard(q);
  const size_t bytes = q->n * sizeof(G1Affine);
  if (hipMalloc(&q->g, bytes) != hipSuccess || hipMalloc(&q->g_lagrange, bytes) != hipSuccess)
    return c->fail(CQ_ERR_HIP, "hipMalloc(params)");
  CQ_HIP(c, hipMemcpyAsync(q->g, p->g, bytes, hipMemcpyDeviceToDevice, c->stream));
  int rc = g1_to_lagrange(c, q->g, k, q->g_lagrange);
  if (rc != CQ_OK) return rc;
  if (c->msm_precompute) {
    if ((rc = msm_register_tables(c, q->g, q->n)) != CQ_OK) return rc;
    if ((rc = msm_register_tables(c, q->g_lagrange, q->n)) != CQ_OK) return rc;
  }
  q->has_g2 = p->has_g2;  // downsize shortens g and g_lagrange in place: g2 and s_g2 stay (commitment.rs:480-492)
  memcpy(q->g2, p->g2, sizeof(q->g2));
  memcpy(q->s_g2, p->s_g2, sizeof(q->s_g2));
  *out = guard.release();
  return CQ_OK;
}

/* G1 part of ParamsKZG::write_custom(RawBytes) (commitment.rs:366-379): 4 + 128 n bytes; cq_params_write_full
 * appends g2 / s_g2. */
int cq_params_write_raw(cq_params* p, uint8_t* buf, size_t cap, size_t* written) {
  if (!p || !buf || !written) return CQ_ERR_ARG;
  cq_ctx* c = p->ctx;
  const size_t bytes = p->n * sizeof(G1Affine);
  if (cap < 4 + 2 * bytes) return c->fail(CQ_ERR_ARG, "params: output buffer too small");
  memcpy(buf, &p->k, 4);
  CQ_HIP(c, hipMemcpyAsync(buf + 4, p->g, bytes, hipMemcpyDeviceToHost, c->stream));
  CQ_HIP(c, hipMemcpyAsync(buf + 4 + bytes, p->g_lagrange, bytes, hipMemcpyDeviceToHost, c->stream));
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  *written = 4 + 2 * bytes;
  return CQ_OK;
}

// A proving key refers to the params (and table config) it was built on for as long as it lives -- it counts itself as a
// user, shares their window tables, restores them when it stops sharding.  The documented order is keys first; a caller
// (or a garbage collector) that destroys the params first only marks them released, and the last key frees them.
void cq_params_destroy(cq_params* p) {
  if (!p) return;
  if (p->key_users > 0) {
    p->owner_released = true;
    return;
  }
  hipStreamSynchronize(p->ctx->stream);
  if (p->g) msm_unregister_tables(p->ctx, p->g);
  if (p->g_lagrange) msm_unregister_tables(p->ctx, p->g_lagrange);
  if (p->g) hipFree(p->g);
  if (p->g_lagrange) hipFree(p->g_lagrange);
  delete p;
}

const uint64_t* cq_params_g_dev(const cq_params* p) { return p ? (const uint64_t*)p->g : nullptr; }
const uint64_t* cq_params_g_lagrange_dev(const cq_params* p) { return p ? (const uint64_t*)p->g_lagrange : nullptr; }

static int commit_host(cq_params* p, const G1Affine* bases, const uint64_t* poly, size_t len, uint64_t out_jac[12]) {
  if (!p || !out_jac || (len && !poly)) return CQ_ERR_ARG;
  cq_ctx* c = p->ctx;
  if (len > p->n) return c->fail(CQ_ERR_ARG, "commit: polynomial longer than the SRS");
  CQ_HIP(c, hipSetDevice(c->device));
  if (len == 0) {
    memset(out_jac, 0, 12 * sizeof(uint64_t));
    return CQ_OK;
  }
  void* ds;
  int rc;
  if ((rc = c->ensure_scratch(Scratch::EntryA, len * sizeof(Fr), &ds)) != CQ_OK) return rc;
  CQ_HIP(c, hipMemcpyAsync(ds, poly, len * sizeof(Fr), hipMemcpyHostToDevice, c->stream));
  const Fr* sc = (const Fr*)ds;
  return msm_batch(c, &sc, bases, len, 1, out_jac);
}

int cq_commit(cq_params* p, const uint64_t* poly, size_t len, uint64_t out_jac[12]) {
  return commit_host(p, p ? p->g : nullptr, poly, len, out_jac);
}
int cq_commit_lagrange(cq_params* p, const uint64_t* poly, size_t len, uint64_t out_jac[12]) {
  return commit_host(p, p ? p->g_lagrange : nullptr, poly, len, out_jac);
}
int cq_commit_dev(cq_params* p, const uint64_t* poly_dev, size_t len, uint64_t out_jac[12]) {
  if (!p || len > p->n) return CQ_ERR_ARG;
  return cq_best_multiexp_dev(p->ctx, poly_dev, (const uint64_t*)p->g, len, out_jac);
}
int cq_commit_lagrange_dev(cq_params* p, const uint64_t* poly_dev, size_t len, uint64_t out_jac[12]) {
  if (!p || len > p->n) return CQ_ERR_ARG;
  return cq_best_multiexp_dev(p->ctx, poly_dev, (const uint64_t*)p->g_lagrange, len, out_jac);
}

}  // extern "C"

extern "C" {
/* sum of `count` Jacobian points (host memory): the local EC sum after an all-gather of per-rank MSM
 * partials (EC addition is not an RCCL reduction op). */
int cq_g1_sum(const uint64_t* jac_points, size_t count, uint64_t out_jac[12]) {
  if ((!jac_points && count) || !out_jac) return CQ_ERR_ARG;
  G1Jac acc = G1Jac::identity();
  for (size_t i = 0; i < count; i++) {
    const uint64_t* p = jac_points + 12 * i;
    G1Jac q = {Fq::from_limbs64(p), Fq::from_limbs64(p + 4), Fq::from_limbs64(p + 8)};
    acc = jac_add(acc, q);
  }
  acc.x.to_limbs64(out_jac);
  acc.y.to_limbs64(out_jac + 4);
  acc.z.to_limbs64(out_jac + 8);
  return CQ_OK;
}
/* `to_affine` (derive/curve.rs:399-412) on the host */
int cq_g1_to_affine(const uint64_t jac[12], uint64_t out_affine[8]) {
  if (!jac || !out_affine) return CQ_ERR_ARG;
  G1Jac q = {Fq::from_limbs64(jac), Fq::from_limbs64(jac + 4), Fq::from_limbs64(jac + 8)};
  G1Affine a = jac_to_affine(q);
  a.x.to_limbs64(out_affine);
  a.y.to_limbs64(out_affine + 4);
  return CQ_OK;
}
}

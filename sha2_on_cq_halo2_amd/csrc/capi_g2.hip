// C ABI: G2 multiexp, the G2 SRS of the table setup and StaticTableValues::commit (the verifying key's
// StaticCommittedTable, plonk/static_lookup.rs:128-157).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include "cq.hpp"
#include "ctx.hpp"
#include "msm_g2.hpp"
#include "plonk.hpp"
#include "poly.hpp"
#include "serde.hpp"

using namespace cq;

// TableSRS's G2 powers (poly/kzg/commitment.rs:73-123, the `g2` vector), resident in HBM
struct cq_g2_srs {
  cq_ctx* ctx;
  size_t count;
  G2Affine* pts = nullptr;
};

namespace {

void jac_out(const G2Jac& p, uint64_t* out) {
  if (p.is_identity()) {
    memset(out, 0, 24 * sizeof(uint64_t));
    return;
  }
  g2_jac_to_limbs64(p, out);
}

void affine_out(const G2Affine& a, uint64_t* out) {
  a.x.to_limbs64(out);
  a.y.to_limbs64(out + 8);
}

// Fq limbs below the modulus (a Montgomery value the reference could have written)
bool fq_limbs_ok(const uint64_t* l) {
  for (int i = 3; i >= 0; i--) {
    const uint64_t m = (uint64_t)FqP::MOD[2 * i] | ((uint64_t)FqP::MOD[2 * i + 1] << 32);
    if (l[i] != m) return l[i] < m;
  }
  return false;
}

G2Affine affine_in(const uint64_t* p) { return {Fq2::from_limbs64(p), Fq2::from_limbs64(p + 8)}; }

uint32_t log2u(size_t x) {
  uint32_t l = 0;
  while (((size_t)1 << (l + 1)) <= x) l++;
  return l;
}

}  // namespace

extern "C" {

// ---- best_multiexp over G2Affine ----------------------------------------------------------------------------------
int cq_best_multiexp_g2_dev(cq_ctx* c, const uint64_t* coeffs_dev, const uint64_t* bases_dev, size_t len, uint64_t out_jac[24]) {
  if (!c || !out_jac || (len && (!coeffs_dev || !bases_dev))) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  G2Jac r;
  const int rc = g2_msm(c, (const Fr*)coeffs_dev, (const G2Affine*)bases_dev, len, &r);
  if (rc != CQ_OK) return rc;
  jac_out(r, out_jac);
  return CQ_OK;
}

int cq_best_multiexp_g2(cq_ctx* c, const uint64_t* coeffs, const uint64_t* bases, size_t len, uint64_t out_jac[24]) {
  if (!c || !out_jac || (len && (!coeffs || !bases))) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  if (len == 0) {
    memset(out_jac, 0, 24 * sizeof(uint64_t));
    return CQ_OK;
  }
  void *ds, *db;
  int rc;
  if ((rc = c->ensure_scratch(Scratch::EntryA, len * sizeof(Fr), &ds)) != CQ_OK) return rc;
  if ((rc = c->ensure_scratch(Scratch::EntryB, len * sizeof(G2Affine), &db)) != CQ_OK) return rc;
  CQ_HIP(c, hipMemcpyAsync(ds, coeffs, len * sizeof(Fr), hipMemcpyHostToDevice, c->stream));
  CQ_HIP(c, hipMemcpyAsync(db, bases, len * sizeof(G2Affine), hipMemcpyHostToDevice, c->stream));
  G2Jac r;
  if ((rc = g2_msm(c, (const Fr*)ds, (const G2Affine*)db, len, &r)) != CQ_OK) return rc;
  jac_out(r, out_jac);
  return CQ_OK;
}

int cq_g2_sum(const uint64_t* jac_points, size_t count, uint64_t out_jac[24]) {
  if ((!jac_points && count) || !out_jac) return CQ_ERR_ARG;
  G2Jac acc = G2Jac::identity();
  for (size_t i = 0; i < count; i++) acc = g2_jac_add(acc, g2_jac_from_limbs64(jac_points + 24 * i));
  jac_out(acc, out_jac);
  return CQ_OK;
}

int cq_g2_to_affine(const uint64_t jac[24], uint64_t out_affine[16]) {
  if (!jac || !out_affine) return CQ_ERR_ARG;
  affine_out(g2_jac_to_affine(g2_jac_from_limbs64(jac)), out_affine);
  return CQ_OK;
}

// ---- G2 SRS -------------------------------------------------------------------------------------------------------
void cq_g2_srs_destroy(cq_g2_srs* s) {
  if (!s) return;
  hipStreamSynchronize(s->ctx->stream);
  if (s->pts) hipFree(s->pts);
  delete s;
}

static int g2_srs_alloc(cq_ctx* c, size_t count, cq_g2_srs** out) {
  cq_g2_srs* s = new cq_g2_srs();
  s->ctx = c;
  s->count = count;
  const hipError_t e = hipMalloc(&s->pts, (count ? count : 1) * sizeof(G2Affine));
  if (e != hipSuccess) {
    s->pts = nullptr;
    delete s;
    return c->hip_fail(e, "hipMalloc(g2 srs)");
  }
  *out = s;
  return CQ_OK;
}

int cq_g2_srs_create(cq_ctx* c, size_t count, const uint64_t* points, int checked, cq_g2_srs** out) {
  if (!c || !out || (count && !points) || count > ((size_t)1 << 30)) return CQ_ERR_ARG;
  *out = nullptr;
  if (checked) {  // as the RawBytes reads of G1: canonical limbs and on the curve (identity allowed)
    const Fq2 b = g2_b();
    for (size_t i = 0; i < count; i++) {
      const uint64_t* p = points + 16 * i;
      for (int k = 0; k < 4; k++)
        if (!fq_limbs_ok(p + 4 * k)) return c->fail(CQ_ERR_ARG, "g2 srs: coordinate not below the modulus");
      if (!g2_on_curve(affine_in(p), b)) return c->fail(CQ_ERR_ARG, "g2 srs: point not on the twist");
    }
  }
  CQ_HIP(c, hipSetDevice(c->device));
  cq_g2_srs* s;
  int rc = g2_srs_alloc(c, count, &s);
  if (rc != CQ_OK) return rc;
  if (count && hipMemcpy(s->pts, points, count * sizeof(G2Affine), hipMemcpyHostToDevice) != hipSuccess) {
    cq_g2_srs_destroy(s);
    return c->fail(CQ_ERR_HIP, "hipMemcpy(g2 srs)");
  }
  *out = s;
  return CQ_OK;
}

int cq_g2_srs_setup_from_toxic_waste(cq_ctx* c, size_t count, const uint64_t s_[4], cq_g2_srs** out) {
  if (!c || !s_ || !out || count > ((size_t)1 << 30)) return CQ_ERR_ARG;
  *out = nullptr;
  CQ_HIP(c, hipSetDevice(c->device));
  cq_g2_srs* s;
  int rc = g2_srs_alloc(c, count, &s);
  if (rc != CQ_OK) return rc;
  if ((rc = g2_srs_powers(c, Fr::from_limbs64(s_), (uint32_t)count, s->pts)) != CQ_OK) {
    cq_g2_srs_destroy(s);
    return rc;
  }
  *out = s;
  return CQ_OK;
}

int cq_g2_srs_download(cq_g2_srs* s, uint64_t* points) {
  if (!s || (s->count && !points)) return CQ_ERR_ARG;
  cq_ctx* c = s->ctx;
  CQ_HIP(c, hipMemcpyAsync(points, s->pts, s->count * sizeof(G2Affine), hipMemcpyDeviceToHost, c->stream));
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  return CQ_OK;
}

size_t cq_g2_srs_len(const cq_g2_srs* s) { return s ? s->count : 0; }

// ---- the G2 SRS as a byte stream: `count` points back to back, `SerdeCurveAffine::write` each (helpers.rs) ------------------
static size_t g2_srs_point_size(int format) {
  if (format == CQ_SERDE_PROCESSED) return 64;
  if (format == CQ_SERDE_RAW_BYTES || format == CQ_SERDE_RAW_BYTES_UNCHECKED) return sizeof(G2Affine);
  return 0;
}
// points converted per staging of compressed bytes: 64 MiB of entry scratch at most
static constexpr size_t G2_SRS_CHUNK = (size_t)1 << 20;

size_t cq_g2_srs_serialized_size(const cq_g2_srs* s, int format) { return s ? s->count * g2_srs_point_size(format) : 0; }

int cq_g2_srs_read(cq_ctx* c, const uint8_t* buf, size_t len, int format, cq_g2_srs** out) {
  if (!c || !out || (len && !buf)) return CQ_ERR_ARG;
  *out = nullptr;
  const size_t psz = g2_srs_point_size(format);
  if (!psz) return c->fail(CQ_ERR_ARG, "g2 srs: unknown serde format");
  if (len % psz) return c->fail(CQ_ERR_ARG, "g2 srs: stream length is not a multiple of the point size");
  const size_t count = len / psz;
  if (count > ((size_t)1 << 30)) return c->fail(CQ_ERR_ARG, "g2 srs: too many points");
  CQ_HIP(c, hipSetDevice(c->device));
  cq_g2_srs* s;
  int rc = g2_srs_alloc(c, count, &s);
  if (rc != CQ_OK) return rc;
  struct Guard {
    cq_g2_srs* s;
    ~Guard() {
      if (s) cq_g2_srs_destroy(s);
    }
  } guard{s};
  if (count == 0) {
    guard.s = nullptr;
    *out = s;
    return CQ_OK;
  }
  if (format != CQ_SERDE_PROCESSED) CQ_HIP(c, hipMemcpyAsync(s->pts, buf, len, hipMemcpyHostToDevice, c->stream));
  if (format != CQ_SERDE_RAW_BYTES_UNCHECKED) {
    void* cells;
    if ((rc = c->ensure_scratch(Scratch::EntryA, 64, &cells)) != CQ_OK) return rc;
    uint32_t* count_dev = (uint32_t*)cells;
    uint32_t* first_dev = count_dev + 1;
    if ((rc = serde_verdict_reset(c, count_dev, first_dev, 1)) != CQ_OK) return rc;
    if (format == CQ_SERDE_PROCESSED) {
      // chunk by chunk through one staging buffer (copies and kernels follow one another on the stream); the kernel reports
      // indices in the whole array
      void* stage;
      if ((rc = c->ensure_scratch(Scratch::EntryB, std::min(count, G2_SRS_CHUNK) * 64, &stage)) != CQ_OK) return rc;
      for (size_t off = 0; off < count; off += G2_SRS_CHUNK) {
        const size_t m = std::min(G2_SRS_CHUNK, count - off);
        CQ_HIP(c, hipMemcpyAsync(stage, buf + off * 64, m * 64, hipMemcpyHostToDevice, c->stream));
        if ((rc = g2_decompress(c, (const uint8_t*)stage, (uint32_t)m, (uint32_t)off, s->pts + off, count_dev, first_dev)) != CQ_OK) return rc;
      }
    } else if ((rc = g2_validate(c, s->pts, (uint32_t)count, 0, count_dev, first_dev)) != CQ_OK) {
      return rc;
    }
    uint32_t verdict[2] = {0, 0};
    CQ_HIP(c, hipMemcpyAsync(verdict, cells, sizeof(verdict), hipMemcpyDeviceToHost, c->stream));
    CQ_HIP(c, hipStreamSynchronize(c->stream));
    if (verdict[0])
      return c->fail(CQ_ERR_ARG, std::string("g2 srs: invalid point ") + (format == CQ_SERDE_PROCESSED ? "encoding" : "(coordinate not below the modulus or not on the twist)") +
                                     " at index " + std::to_string(verdict[1]) + " (" + std::to_string(verdict[0]) + " invalid in all)");
  }
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  guard.s = nullptr;
  *out = s;
  return CQ_OK;
}

int cq_g2_srs_write(cq_g2_srs* s, int format, uint8_t* buf, size_t cap, size_t* written) {
  if (!s || !written || (s->count && !buf)) return CQ_ERR_ARG;
  cq_ctx* c = s->ctx;
  const size_t psz = g2_srs_point_size(format);
  if (!psz) return c->fail(CQ_ERR_ARG, "g2 srs: unknown serde format");
  if (cap < s->count * psz) return c->fail(CQ_ERR_ARG, "g2 srs: output buffer too small");
  CQ_HIP(c, hipSetDevice(c->device));
  if (format != CQ_SERDE_PROCESSED) {
    CQ_HIP(c, hipMemcpyAsync(buf, s->pts, s->count * psz, hipMemcpyDeviceToHost, c->stream));
  } else if (s->count) {
    void* stage;
    int rc;
    if ((rc = c->ensure_scratch(Scratch::EntryB, std::min(s->count, G2_SRS_CHUNK) * 64, &stage)) != CQ_OK) return rc;
    for (size_t off = 0; off < s->count; off += G2_SRS_CHUNK) {
      const size_t m = std::min(G2_SRS_CHUNK, s->count - off);
      if ((rc = g2_compress(c, s->pts + off, (uint32_t)m, (uint8_t*)stage)) != CQ_OK) return rc;
      CQ_HIP(c, hipMemcpyAsync(buf + off * 64, stage, m * 64, hipMemcpyDeviceToHost, c->stream));
    }
  }
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  *written = s->count * psz;
  return CQ_OK;
}

const uint64_t* cq_g2_srs_dev(const cq_g2_srs* s) { return s ? (const uint64_t*)s->pts : nullptr; }

// ---- StaticTableValues::commit (static_lookup.rs:128-157) ------------------------------------------------------------
int cq_static_table_commit(cq_static_table* table, cq_g2_srs* srs, size_t srs_g1_len, size_t circuit_n, uint64_t zv[16],
                           uint64_t t[16], uint64_t x_b0_bound[16]) {
  if (!table || !srs || !zv || !t || !x_b0_bound || srs->ctx != table->ctx) return CQ_ERR_ARG;
  cq_ctx* c = table->ctx;
  const size_t N = table->N;
  // the reference indexes srs_g2[N] and srs_g2[srs_g1_len - 1 - (circuit_n - 2)] (it would panic out of range)
  if (srs->count < N + 1) return c->fail(CQ_ERR_ARG, "static table commit: G2 SRS shorter than N + 1");
  if (circuit_n < 2 || srs_g1_len + 1 < circuit_n || srs_g1_len + 1 - circuit_n >= srs->count)
    return c->fail(CQ_ERR_ARG, "static table commit: x_b0_bound index out of range");
  const size_t bound_idx = srs_g1_len + 1 - circuit_n;
  CQ_HIP(c, hipSetDevice(c->device));
  // t: the iNTT of the table's values in ascending canonical order (value_index_mapping.keys(), a BTreeMap), then
  // best_multiexp over srs_g2[..N]
  uint64_t* keys = nullptr;
  CQ_HIP(c, hipMalloc(&keys, N * 8 * sizeof(uint64_t)));
  Fr* sorted = (Fr*)(keys + 4 * N);
  Fr* coeffs = (Fr*)keys;  // the keys are dead once converted back
  cq_domain* dom = nullptr;
  G2Jac tj;
  int rc = fr_to_canonical(c, table->values, (uint32_t)N, keys);
  if (rc == CQ_OK) rc = sort_canonical_dev(c, keys, (uint32_t)N);
  if (rc == CQ_OK) rc = fr_from_canonical(c, keys, (uint32_t)N, sorted);
  if (rc == CQ_OK) rc = domain_create(c, 2, log2u(N), &dom);
  if (rc == CQ_OK) rc = domain_lagrange_to_coeff(dom, sorted, coeffs, 1, N, N);
  if (rc == CQ_OK) rc = g2_msm(c, coeffs, srs->pts, N, &tj);
  hipStreamSynchronize(c->stream);
  if (dom) domain_destroy(dom);
  hipFree(keys);
  if (rc != CQ_OK) return rc;
  // zv = srs_g2[N] - srs_g2[0];  x_b0_bound = srs_g2[srs_g1_len - 1 - (circuit_n - 2)]
  G2Affine p0, pn, pb;
  CQ_HIP(c, hipMemcpy(&p0, srs->pts, sizeof(G2Affine), hipMemcpyDeviceToHost));
  CQ_HIP(c, hipMemcpy(&pn, srs->pts + N, sizeof(G2Affine), hipMemcpyDeviceToHost));
  CQ_HIP(c, hipMemcpy(&pb, srs->pts + bound_idx, sizeof(G2Affine), hipMemcpyDeviceToHost));
  affine_out(g2_jac_to_affine(g2_jac_add(g2_jac_from_affine(pn), g2_jac_neg(g2_jac_from_affine(p0)))), zv);
  affine_out(g2_jac_to_affine(tj), t);
  affine_out(pb, x_b0_bound);
  return CQ_OK;
}

}  // extern "C"

// Proving key: construction (keygen, or ProvingKey::read in the three serde formats), ProvingKey::write, the key's MSM window
// tables and their re-tabling under sharding, destruction.  The other cq_pk_* entry points (opener, RNG, proof size,
// commitments) and create_proof are in capi_cq.hip.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include "building.hpp"
#include "cq.hpp"
#include "ctx.hpp"
#include "g1fft.hpp"
#include "msm.hpp"
#include "plonk.hpp"
#include "poly.hpp"
#include "serde.hpp"

using namespace cq;

size_t cq::static_table_rows(const cq_static_table* t) { return t->N; }

namespace {
void put_be32(uint8_t*& o, uint32_t v) {
  o[0] = (uint8_t)(v >> 24); o[1] = (uint8_t)(v >> 16); o[2] = (uint8_t)(v >> 8); o[3] = (uint8_t)v;
  o += 4;
}
// unit vector at `row` on the extended coset (l0 / l_last, keygen.rs:340-363); tmp: n elements of scratch
int unit_coset(cq_pk* pk, size_t row, Fr* tmp, Fr* dst) {
  cq_ctx* c = pk->ctx;
  const size_t n = (size_t)1 << pk->k, ext = pk->domain->ext();
  const Fr one = Fr::one();
  CQ_HIP(c, hipMemsetAsync(tmp, 0, n * sizeof(Fr), c->stream));
  CQ_HIP(c, hipMemcpyAsync(tmp + row, &one, sizeof(Fr), hipMemcpyHostToDevice, c->stream));
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  int rc;
  if ((rc = domain_lagrange_to_coeff(pk->domain, tmp, tmp, 1, n, n)) != CQ_OK) return rc;
  return domain_coeff_to_extended(pk->domain, tmp, dst, 1, n, ext);
}
}  // namespace

// Window tables of the arrays a key multiplies over besides its SRS, at the width of the SRS tables (so that all MSMs of
// a round share one launch): the cached quotients and an own b0 bound are the key's; the table SRS may be shared with
// keys of other sizes and then carries a table per width (2^12 points: 4 MiB each).  The width follows the length of
// the point range a rank multiplies: 2^k / world.
static int pk_small_tables(cq_pk* pk) {
  cq_ctx* c = pk->ctx;
  const size_t n = (size_t)1 << pk->k;
  const uint32_t width = c->msm_table_c ? c->msm_table_c : msm_table_window_bits(n / std::max<uint32_t>(pk->shard_world, 1));
  if (width == pk->table_c && !pk->held_tables.empty()) return CQ_OK;
  pk->table_c = width;
  if (!c->msm_precompute) return CQ_OK;
  std::vector<cq_pk::TableRef> old;
  old.swap(pk->held_tables);
  int rc = CQ_OK;
  auto want = [&](const G1Affine* b, size_t len) {
    bool held = false;
    if (rc == CQ_OK) rc = msm_register_tables(c, b, len, pk->table_c, &held);
    if (held) pk->held_tables.push_back({b, len, pk->table_c});
  };
  const cq_table_config* cfg = pk->table_cfg;
  for (size_t l = 0; l < pk->qs_concat.size(); l++) want(pk->qs_concat[l], pk->lookups[l].tables.size() * cfg->N);
  if (cfg && !pk->lookups.empty()) {
    want(cfg->g1_lagrange, cfg->N);
    want(cfg->g_lagrange_opening_at_0, cfg->N);
  }
  if (pk->b0_g1_bound) want(pk->b0_g1_bound, n - 1);
  for (auto& t : old) msm_release_table(c, t.bases, t.n, t.c);  // after the new ones: a shared entry is never rebuilt in between
  return rc;
}

// ---- construction ------------------------------------------------------------------------------------
// cq_pk_create / cq_pk_read* in five steps ("Key construction"): describe (pk.hpp, host only), upload the expression
// programs, allocate the key's polynomials, fill them -- computed (pk_keygen_polys) or read from a stream (pk_read_polys) --
// and attach the G1 arrays.
template <class T>
static int upload_new(cq_ctx* c, T** dst, const T* src, size_t count, const char* what) {
  int rc = c->dev_alloc(dst, count, what);
  if (rc != CQ_OK) return rc;
  CQ_HIP(c, hipMemcpy(*dst, src, count * sizeof(T), hipMemcpyHostToDevice));
  return CQ_OK;
}

static int pk_upload_programs(cq_pk* pk, const cq_plonk* pl) {
  if (!pl) return CQ_OK;
  cq_ctx* c = pk->ctx;
  const PkPrograms prog = pk_pack_programs(pl, pk);
  int rc;
  if (!prog.gates.empty() && (rc = upload_new(c, &pk->gate_prog, prog.gates.data(), prog.gates.size(), "gate program")) != CQ_OK) return rc;
  if (pl->num_constants && (rc = upload_new(c, &pk->constants, (const Fr*)pl->constants, pl->num_constants, "gate constants")) != CQ_OK) return rc;
  if (!prog.legacy.empty() && (rc = upload_new(c, &pk->legacy_prog, prog.legacy.data(), prog.legacy.size(), "legacy lookup programs")) != CQ_OK)
    return rc;
  if (!prog.lookups.empty() && (rc = upload_new(c, &pk->lookup_prog, prog.lookups.data(), prog.lookups.size(), "lookup programs")) != CQ_OK) return rc;
  return CQ_OK;
}

// Every Fr array of the key, for keygen and for the readers alike, and the powers of omega that neither path takes from a stream
static int pk_alloc_polys(cq_pk* pk) {
  cq_ctx* c = pk->ctx;
  const size_t n = (size_t)1 << pk->k, ext = pk->domain->ext(), F = pk->num_fixed, PC = pk->perm_columns.size();
  int rc;
  if ((rc = c->dev_alloc(&pk->l_active_row, ext, "l_active_row")) != CQ_OK) return rc;
  if (pk->general() && ((rc = c->dev_alloc(&pk->l0, ext, "l0/l_last")) != CQ_OK || (rc = c->dev_alloc(&pk->l_last, ext, "l0/l_last")) != CQ_OK)) return rc;
  if (F && ((rc = c->dev_alloc(&pk->fixed_values, F * n, "fixed columns")) != CQ_OK || (rc = c->dev_alloc(&pk->fixed_polys, F * n, "fixed columns")) != CQ_OK ||
            (rc = c->dev_alloc(&pk->fixed_cosets, F * ext, "fixed columns")) != CQ_OK))
    return rc;
  if (!PC) return CQ_OK;
  const size_t hi = std::max<size_t>(ext / 256, 1);
  if ((rc = c->dev_alloc(&pk->omega_powers, n, "permutation key")) != CQ_OK || (rc = c->dev_alloc(&pk->perm_values, PC * n, "permutation key")) != CQ_OK ||
      (rc = c->dev_alloc(&pk->perm_polys, PC * n, "permutation key")) != CQ_OK || (rc = c->dev_alloc(&pk->perm_cosets, PC * ext, "permutation key")) != CQ_OK ||
      (rc = c->dev_alloc(&pk->ext_pow_lo, 256, "extended omega powers")) != CQ_OK || (rc = c->dev_alloc(&pk->ext_pow_hi, hi, "extended omega powers")) != CQ_OK)
    return rc;
  if ((rc = fr_powers(c, pk->domain->omega, (uint32_t)n, pk->omega_powers)) != CQ_OK ||
      (rc = fr_powers(c, pk->domain->extended_omega, 256, pk->ext_pow_lo)) != CQ_OK)
    return rc;
  return fr_powers(c, pk->domain->extended_omega.pow_u64(256), (uint32_t)hi, pk->ext_pow_hi);
}

// keygen_pk (plonk/keygen.rs:278-397): the key's polynomials computed from the description
static int pk_keygen_polys(cq_pk* pk, const cq_plonk* pl) {
  cq_ctx* c = pk->ctx;
  const size_t n = (size_t)1 << pk->k, ext = pk->domain->ext(), F = pk->num_fixed, PC = pk->perm_columns.size();
  void* scratch;
  int rc;
  if ((rc = c->ensure_scratch(Scratch::EntryA, n * sizeof(Fr), &scratch)) != CQ_OK) return rc;
  Fr* tmp = (Fr*)scratch;
  // l_active_row = 1 - (l_last + l_blind) on the extended coset (keygen.rs:344-373); by linearity it is
  // the coset extension of the indicator of the usable rows
  if ((rc = poly_fill_usable_rows(c, tmp, (uint32_t)n, pk->u)) != CQ_OK) return rc;
  if ((rc = domain_lagrange_to_coeff(pk->domain, tmp, tmp, 1, n, n)) != CQ_OK) return rc;
  if ((rc = domain_coeff_to_extended(pk->domain, tmp, pk->l_active_row, 1, n, ext)) != CQ_OK) return rc;
  // l0 (keygen.rs:340-345) and l_last (:357-363): unit vectors at rows 0 and n - bf - 1
  if (pk->general() && ((rc = unit_coset(pk, 0, tmp, pk->l0)) != CQ_OK || (rc = unit_coset(pk, n - pk->bf - 1, tmp, pk->l_last)) != CQ_OK)) return rc;
  if (F) {
    for (size_t f = 0; f < F; f++)
      CQ_HIP(c, hipMemcpyAsync(pk->fixed_values + f * n, pl->fixed[f], n * sizeof(Fr), hipMemcpyHostToDevice, c->stream));
    if ((rc = domain_lagrange_to_coeff(pk->domain, pk->fixed_values, pk->fixed_polys, (uint32_t)F, n, n)) != CQ_OK) return rc;
    if ((rc = domain_coeff_to_extended(pk->domain, pk->fixed_polys, pk->fixed_cosets, (uint32_t)F, n, ext)) != CQ_OK) return rc;
  }
  if (!PC) return CQ_OK;
  // permutation::keygen::Assembly::build_pk (permutation/keygen.rs:151-208)
  std::vector<uint32_t> ident;
  const uint32_t* mapping = pl->perm_mapping;  // (range-checked by pk_describe)
  if (!mapping) {
    ident.resize(PC * n * 2);
    for (size_t col = 0; col < PC; col++)
      for (size_t r = 0; r < n; r++) {
        ident[(col * n + r) * 2] = (uint32_t)col;
        ident[(col * n + r) * 2 + 1] = (uint32_t)r;
      }
    mapping = ident.data();
  }
  std::vector<Fr> dp(PC);
  const Fr delta = fr_from_raw(FR_DELTA_RAW);
  Fr cur = Fr::one();
  for (size_t col = 0; col < PC; col++) {
    dp[col] = cur;
    cur = cur * delta;
  }
  void* stage;
  if ((rc = c->ensure_scratch(Scratch::EntryB, PC * n * 2 * sizeof(uint32_t) + PC * sizeof(Fr), &stage)) != CQ_OK) return rc;
  Fr* dp_dev = (Fr*)stage;
  uint32_t* map_dev = (uint32_t*)(dp_dev + PC);
  CQ_HIP(c, hipMemcpy(dp_dev, dp.data(), PC * sizeof(Fr), hipMemcpyHostToDevice));
  CQ_HIP(c, hipMemcpy(map_dev, mapping, PC * n * 2 * sizeof(uint32_t), hipMemcpyHostToDevice));
  if ((rc = perm_sigma(c, map_dev, (uint32_t)PC, (uint32_t)n, pk->omega_powers, dp_dev, pk->perm_values)) != CQ_OK) return rc;
  if ((rc = domain_lagrange_to_coeff(pk->domain, pk->perm_values, pk->perm_polys, (uint32_t)PC, n, n)) != CQ_OK) return rc;
  return domain_coeff_to_extended(pk->domain, pk->perm_polys, pk->perm_cosets, (uint32_t)PC, n, ext);
}

namespace {
// Reader of a ProvingKey::write byte stream (plonk.rs:349-403) in any SerdeFormat: big-endian u32 counts, 32-byte elements
// uploaded straight to where the key keeps them and converted (Processed) or validated (RawBytes) there.
// begin() takes the words the device reports through -- the Processed verdicts, [0] the commitments and [1 + j] polynomial j
// of the stream, or the one flag of RawBytes -- from Scratch::EntryA, once and sized for the whole stream; finish() reads them
// back.  A scratch buffer that grows is freed, so NOTHING between begin() and finish() may ask for EntryA: poly() and
// slice() stage through EntryB alone, and pk_read_polys calls nothing else in between.
struct PkStreamReader {
  const uint8_t* p;
  size_t left;
  uint32_t num_selectors;
  bool checked, processed;  // RawBytes / Processed; neither: RawBytesUnchecked
  cq_ctx* c = nullptr;
  bool ok = true;
  size_t poly_index = 0, cells = 0;
  uint32_t *count_dev = nullptr, *first_dev = nullptr;  // `cells` words each; count_dev[0] doubles as the RawBytes flag
  std::vector<std::pair<Fr*, size_t>> to_check;         // uploaded vectors to validate under RawBytes

  uint32_t be32() {
    if (left < 4) { ok = false; return 0; }
    const uint32_t v = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
    p += 4;
    left -= 4;
    return v;
  }
  const uint8_t* take(size_t bytes) {
    if (left < bytes) { ok = false; return nullptr; }
    const uint8_t* q = p;
    p += bytes;
    left -= bytes;
    return q;
  }
  // The VerifyingKey part (k, fixed / permutation commitments, selector bits; plonk.rs:92-113) is checked against the key's
  // shape and skipped: the prover only needs the shape, which the circuit description gives.
  int begin(const cq_pk* pk) {
    c = pk->ctx;
    const size_t n = (size_t)1 << pk->k;
    const uint32_t rk = be32(), nfix = be32();
    const size_t ncm = (size_t)nfix + pk->perm_columns.size(), cm_bytes = ncm * (processed ? 32 : sizeof(G1Affine));
    const uint8_t* cm = take(cm_bytes);
    take((size_t)num_selectors * ((n + 7) / 8));
    if (!ok || rk != pk->k || nfix != pk->num_fixed) return c->fail(CQ_ERR_ARG, "pk: serialized key does not match the circuit");
    cells = 4 + 3 * ((size_t)pk->num_fixed + pk->perm_columns.size());
    void* words;
    int rc;
    if ((rc = c->ensure_scratch(Scratch::EntryA, 2 * cells * sizeof(uint32_t), &words)) != CQ_OK) return rc;
    count_dev = (uint32_t*)words;
    first_dev = count_dev + cells;
    if (!processed) return CQ_OK;
    if ((rc = serde_verdict_reset(c, count_dev, first_dev, cells)) != CQ_OK) return rc;
    if (ncm) {  // compressed commitments: decompressed to validate them (`C::read`, plonk.rs:120-127), then dropped
      void* stage;
      if ((rc = c->ensure_scratch(Scratch::EntryB, cm_bytes + ncm * sizeof(G1Affine), &stage)) != CQ_OK) return rc;
      CQ_HIP(c, hipMemcpyAsync(stage, cm, cm_bytes, hipMemcpyHostToDevice, c->stream));
      return g1_decompress(c, (const uint8_t*)stage, (uint32_t)ncm, (G1Affine*)((uint8_t*)stage + cm_bytes), count_dev, first_dev);
    }
    return CQ_OK;
  }
  // one polynomial of `expect` elements into dst; dst == nullptr: a section the prover does not keep (l0 / l_last of a
  // CQ-only key), which Processed still validates, in scratch
  int poly(Fr* dst, size_t expect) {
    const uint32_t len = be32();
    const size_t bytes = (size_t)len * sizeof(Fr);
    const uint8_t* src = take(bytes);
    if (!ok || len != expect) return c->fail(CQ_ERR_ARG, "pk: serialized polynomial has the wrong length");
    const size_t j = poly_index++;
    if (!dst) {
      if (!processed || !len) return CQ_OK;
      int rc = c->ensure_scratch(Scratch::EntryB, bytes, (void**)&dst);
      if (rc != CQ_OK) return rc;
    } else if (!processed) {
      to_check.push_back({dst, len});
    }
    CQ_HIP(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    // canonical scalars: converted where they landed (helpers.rs:68-79)
    return processed ? fr_from_repr(c, (const uint8_t*)dst, len, dst, count_dev + 1 + j, first_dev + 1 + j) : CQ_OK;
  }
  // a slice of `count` polynomials of `each` elements, contiguous at dst (an empty slice has no dst)
  int slice(Fr* dst, size_t count, size_t each) {
    if (be32() != count || !ok) return c->fail(CQ_ERR_ARG, "pk: serialized key has a different number of polynomials");
    for (size_t i = 0; i < count; i++) {
      int rc = poly(dst + i * each, each);
      if (rc != CQ_OK) return rc;
    }
    return CQ_OK;
  }
  int finish() {
    if (left != 0) return c->fail(CQ_ERR_ARG, "pk: trailing bytes after the serialized key");
    if (processed) {  // the verdicts of the conversions
      std::vector<uint32_t> verdict(2 * cells);
      CQ_HIP(c, hipMemcpyAsync(verdict.data(), count_dev, 2 * cells * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
      CQ_HIP(c, hipStreamSynchronize(c->stream));
      if (verdict[0])
        return c->fail(CQ_ERR_ARG, "pk: invalid point encoding at commitment " + std::to_string(verdict[cells]) +
                                       " (fixed commitments first, then permutation commitments)");
      for (size_t j = 1; j < cells; j++)
        if (verdict[j])
          return c->fail(CQ_ERR_ARG, "pk: field element not below the modulus at polynomial " + std::to_string(j - 1) + " element " +
                                         std::to_string(verdict[cells + j]) + " (polynomials in stream order, l0 = 0)");
    } else if (checked) {  // every field element below the modulus (helpers.rs:62-79)
      int rc;
      CQ_HIP(c, hipMemsetAsync(count_dev, 0, 4, c->stream));
      for (auto& v : to_check)
        if ((rc = fr_validate(c, v.first, v.second, count_dev)) != CQ_OK) return rc;
      uint32_t bad = 0;
      CQ_HIP(c, hipMemcpyAsync(&bad, count_dev, 4, hipMemcpyDeviceToHost, c->stream));
      CQ_HIP(c, hipStreamSynchronize(c->stream));
      if (bad) return c->fail(CQ_ERR_ARG, "pk: field element not below the modulus");
    }
    return CQ_OK;
  }
};
}  // namespace

// ProvingKey::read (plonk.rs:379-403): the key's polynomials uploaded straight into HBM instead of being recomputed
static int pk_read_polys(cq_pk* pk, PkStreamReader& rd) {
  const size_t n = (size_t)1 << pk->k, ext = pk->domain->ext(), F = pk->num_fixed, PC = pk->perm_columns.size();
  int rc;
  if ((rc = rd.begin(pk)) != CQ_OK) return rc;
  // l0, l_last, l_active_row (keygen.rs:338-373) come first; a CQ-only prover keeps only the last
  if ((rc = rd.poly(pk->l0, ext)) != CQ_OK || (rc = rd.poly(pk->l_last, ext)) != CQ_OK || (rc = rd.poly(pk->l_active_row, ext)) != CQ_OK) return rc;
  if ((rc = rd.slice(pk->fixed_values, F, n)) != CQ_OK || (rc = rd.slice(pk->fixed_polys, F, n)) != CQ_OK ||
      (rc = rd.slice(pk->fixed_cosets, F, ext)) != CQ_OK)
    return rc;
  // permutation::ProvingKey::read (permutation.rs:124-134)
  if ((rc = rd.slice(pk->perm_values, PC, n)) != CQ_OK || (rc = rd.slice(pk->perm_polys, PC, n)) != CQ_OK ||
      (rc = rd.slice(pk->perm_cosets, PC, ext)) != CQ_OK)
    return rc;
  return rd.finish();
}

// The G1 arrays of the key: b0_g1_bound (n - 1 points: best_multiexp asserts equal lengths, arithmetic.rs:133), the cached
// quotients, the window tables of both and the per-row bases of [b_0] and [p]
static int pk_attach_bases(cq_pk* pk, const uint64_t* b0_g1_bound, int b0_on_device) {
  cq_ctx* c = pk->ctx;
  const cq_table_config* cfg = pk->table_cfg;
  const size_t n = (size_t)1 << pk->k;
  int rc;
  if (b0_g1_bound && b0_on_device) {
    pk->b0_g1_bound = (G1Affine*)b0_g1_bound;
  } else if (b0_g1_bound) {
    if ((rc = c->dev_alloc(&pk->b0_g1_bound, n - 1, "b0 bound")) != CQ_OK) return rc;
    pk->own_b0 = true;
    CQ_HIP(c, hipMemcpyAsync(pk->b0_g1_bound, b0_g1_bound, (n - 1) * sizeof(G1Affine), hipMemcpyHostToDevice, c->stream));
  }
  // per lookup: [qs_0 | qs_1 | ...] so that q_a is one MSM
  for (auto& lk : pk->lookups) {
    G1Affine* cat = nullptr;
    const size_t N = cfg->N;
    if ((rc = c->dev_alloc(&cat, lk.tables.size() * N, "qs")) != CQ_OK) return rc;
    pk->qs_concat.push_back(cat);
    for (size_t j = 0; j < lk.tables.size(); j++)
      CQ_HIP(c, hipMemcpyAsync(cat + j * N, lk.tables[j]->qs, N * sizeof(G1Affine), hipMemcpyDeviceToDevice, c->stream));
  }
  if ((rc = pk_small_tables(pk)) != CQ_OK) return rc;
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  // the per-row bases of [b_0] and [p] (cq.hpp): two G1 transforms, once per key
  if (!pk->lookups.empty() && pk->b0_g1_bound && cfg->N + 1 <= ((size_t)1 << (MSM_TABLE_C - 1)) && n >= 2) {
    const G1Affine* src[2] = {pk->params->g, pk->b0_g1_bound};
    for (int q = 0; q < 2; q++) {
      if ((rc = c->dev_alloc(&pk->b_row_bases[q], n, "b row bases")) != CQ_OK) return rc;
      if ((rc = g1_to_lagrange_shifted(c, src[q], (uint32_t)(n - 1), 1, pk->k, pk->b_row_bases[q])) != CQ_OK) return rc;
      if (msm_bases29(c, pk->b_row_bases[q], (uint32_t)n, pk->b_row_bases[q]) != 0) return c->fail(CQ_ERR_HIP, "b row bases");
    }
    CQ_HIP(c, hipStreamSynchronize(c->stream));
  }
  return CQ_OK;
}

// `in` == nullptr: keygen; otherwise the polynomials come from the stream
static int pk_create_impl(cq_ctx* c, cq_params* params, const cq_circuit* cs, cq_table_config* cfg, const uint64_t* b0_g1_bound,
                          int b0_on_device, PkStreamReader* in, cq_pk** out) {
  if (!c || !params || !cs || !out) return CQ_ERR_ARG;
  *out = nullptr;
  cq_pk_desc desc;
  std::string why;
  int rc = pk_describe(cs, params->k, cfg ? &cfg->N : nullptr, b0_g1_bound != nullptr, in != nullptr,
                       PkLimits{CQ_MAX_LOOKUPS, CQ_MAX_WIDTH, PERM_MAX_COLUMNS, PERM_MAX_CHUNK}, &desc, &why);
  if (rc != CQ_OK) return c->fail(rc, why);
  CQ_HIP(c, hipSetDevice(c->device));
  cq_pk* pk = new cq_pk();
  Building<cq_pk> guard(pk, cq_pk_destroy, c);  // every failing return below (CQ_HIP included) destroys the key
  static_cast<cq_pk_desc&>(*pk) = std::move(desc);
  pk->ctx = c;
  pk->params = params;
  pk->table_cfg = cfg;
  pk->vk_repr = Fr::from_limbs64(cs->vk_repr);
  params->key_users++;
  if (cfg) cfg->key_users++;
  pk->counted_users = true;
  if ((rc = pk_upload_programs(pk, cs->plonk)) != CQ_OK) return rc;
  // extended domain for cs.degree(): 3 for permutation / static lookups (static_lookup.rs:181-190), more with gates
  if ((rc = domain_create(c, pk->cs_degree, pk->k, &pk->domain)) != CQ_OK) return rc;
  if ((rc = pk_alloc_polys(pk)) != CQ_OK) return rc;
  if ((rc = in ? pk_read_polys(pk, *in) : pk_keygen_polys(pk, cs->plonk)) != CQ_OK) return rc;
  if ((rc = pk_attach_bases(pk, b0_g1_bound, b0_on_device)) != CQ_OK) return rc;
  *out = guard.release();
  return CQ_OK;
}

extern "C" {

int cq_pk_create(cq_ctx* c, cq_params* params, const cq_circuit* cs, cq_table_config* cfg, const uint64_t* b0_g1_bound,
                 int b0_on_device, cq_pk** out) {
  return pk_create_impl(c, params, cs, cfg, b0_g1_bound, b0_on_device, nullptr, out);
}

int cq_pk_read_raw(cq_ctx* c, cq_params* params, const cq_circuit* cs, cq_table_config* cfg, const uint64_t* b0_g1_bound,
                   int b0_on_device, const uint8_t* buf, size_t len, uint32_t num_selectors, int checked, cq_pk** out) {
  if (!buf) return CQ_ERR_ARG;
  PkStreamReader in{buf, len, num_selectors, checked != 0, false};
  return pk_create_impl(c, params, cs, cfg, b0_g1_bound, b0_on_device, &in, out);
}

// ProvingKey::read in any SerdeFormat (plonk.rs:379-403)
int cq_pk_read(cq_ctx* c, cq_params* params, const cq_circuit* cs, cq_table_config* cfg, const uint64_t* b0_g1_bound, int b0_on_device,
               const uint8_t* buf, size_t len, uint32_t num_selectors, int format, cq_pk** out) {
  if (!buf) return CQ_ERR_ARG;
  if (format != CQ_SERDE_PROCESSED && format != CQ_SERDE_RAW_BYTES && format != CQ_SERDE_RAW_BYTES_UNCHECKED)
    return c ? c->fail(CQ_ERR_ARG, "pk: unknown serde format") : CQ_ERR_ARG;
  PkStreamReader in{buf, len, num_selectors, format == CQ_SERDE_RAW_BYTES, format == CQ_SERDE_PROCESSED};
  return pk_create_impl(c, params, cs, cfg, b0_g1_bound, b0_on_device, &in, out);
}

static size_t pk_stream_size(const cq_pk* pk, uint32_t num_selectors, size_t point_bytes) {
  if (!pk) return 0;
  const size_t n = (size_t)1 << pk->k, ext = pk->domain->ext(), F = pk->num_fixed, PC = pk->perm_columns.size();
  const size_t poly_n = 4 + n * sizeof(Fr), poly_e = 4 + ext * sizeof(Fr);
  return 8 + (F + PC) * point_bytes + (size_t)num_selectors * ((n + 7) / 8) + 3 * poly_e + 3 * 4 + F * (2 * poly_n + poly_e) + 3 * 4 +
         PC * (2 * poly_n + poly_e);
}
size_t cq_pk_raw_size(const cq_pk* pk, uint32_t num_selectors) { return pk_stream_size(pk, num_selectors, sizeof(G1Affine)); }
// a canonical scalar is as long as a raw one: the formats differ by the commitments alone
size_t cq_pk_serialized_size(const cq_pk* pk, int format, uint32_t num_selectors) {
  if (format == CQ_SERDE_PROCESSED) return pk_stream_size(pk, num_selectors, 32);
  if (format == CQ_SERDE_RAW_BYTES || format == CQ_SERDE_RAW_BYTES_UNCHECKED) return pk_stream_size(pk, num_selectors, sizeof(G1Affine));
  return 0;
}

// ProvingKey::write (plonk.rs:349-362); processed: compressed commitments, canonical scalars (converted into the second
// entry buffer, one polynomial at a time, and copied out from there)
static int pk_write_impl(cq_pk* pk, bool processed, const uint8_t* selector_bits, uint32_t num_selectors, uint8_t* buf, size_t cap,
                         size_t* written) {
  if (!pk || !buf || !written || (num_selectors && !selector_bits)) return CQ_ERR_ARG;
  cq_ctx* c = pk->ctx;
  CQ_HIP(c, hipSetDevice(c->device));
  const size_t n = (size_t)1 << pk->k, ext = pk->domain->ext(), F = pk->num_fixed, PC = pk->perm_columns.size();
  const size_t total = pk_stream_size(pk, num_selectors, processed ? 32 : sizeof(G1Affine));
  if (cap < total) return c->fail(CQ_ERR_ARG, "pk: output buffer too small");
  uint8_t* o = buf;
  // VerifyingKey::write (:92-113): k, fixed commitments, permutation commitments, packed selector bits
  put_be32(o, pk->k);
  put_be32(o, (uint32_t)F);
  std::vector<uint64_t> cm((F + PC) * 8 + 8);
  int rc = cq_pk_vk_commitments(pk, cm.data(), cm.data() + F * 8);
  if (rc != CQ_OK) return rc;
  void* stage = nullptr;  // processed only
  if (processed) {
    if ((rc = c->ensure_scratch(Scratch::EntryB, std::max(ext * sizeof(Fr), (F + PC) * (sizeof(G1Affine) + 32)), &stage)) != CQ_OK) return rc;
    if (F + PC) {
      uint8_t* packed = (uint8_t*)stage + (F + PC) * sizeof(G1Affine);
      CQ_HIP(c, hipMemcpyAsync(stage, cm.data(), (F + PC) * sizeof(G1Affine), hipMemcpyHostToDevice, c->stream));
      if ((rc = g1_compress(c, (const G1Affine*)stage, (uint32_t)(F + PC), packed)) != CQ_OK) return rc;
      CQ_HIP(c, hipMemcpyAsync(o, packed, (F + PC) * 32, hipMemcpyDeviceToHost, c->stream));
      CQ_HIP(c, hipStreamSynchronize(c->stream));
    }
    o += (F + PC) * 32;
  } else {
    memcpy(o, cm.data(), (F + PC) * sizeof(G1Affine));
    o += (F + PC) * sizeof(G1Affine);
  }
  const size_t sel_bytes = (size_t)num_selectors * ((n + 7) / 8);
  if (sel_bytes) memcpy(o, selector_bits, sel_bytes);
  o += sel_bytes;
  auto write_poly = [&](const Fr* src, size_t len) -> int {
    put_be32(o, (uint32_t)len);
    if (processed) {  // (stream order: the next conversion waits for this copy)
      int r2 = fr_to_repr(c, src, (uint32_t)len, (uint8_t*)stage);
      if (r2 != CQ_OK) return r2;
      src = (const Fr*)stage;
    }
    CQ_HIP(c, hipMemcpyAsync(o, src, len * sizeof(Fr), hipMemcpyDeviceToHost, c->stream));
    o += len * sizeof(Fr);
    return CQ_OK;
  };
  auto write_slice = [&](const Fr* src, size_t count, size_t each) -> int {
    put_be32(o, (uint32_t)count);
    for (size_t i = 0; i < count; i++) {
      int r2 = write_poly(src + i * each, each);
      if (r2 != CQ_OK) return r2;
    }
    return CQ_OK;
  };
  // l0, l_last (a CQ-only key does not keep them: computed here), l_active_row
  void* tmp;
  if ((rc = c->ensure_scratch(Scratch::EntryA, (n + 2 * ext) * sizeof(Fr), &tmp)) != CQ_OK) return rc;
  Fr* l0 = pk->l0;
  Fr* l_last = pk->l_last;
  if (!l0) {
    l0 = (Fr*)tmp + n;
    l_last = l0 + ext;
    if ((rc = unit_coset(pk, 0, (Fr*)tmp, l0)) != CQ_OK || (rc = unit_coset(pk, n - pk->bf - 1, (Fr*)tmp, l_last)) != CQ_OK) return rc;
  }
  if ((rc = write_poly(l0, ext)) != CQ_OK || (rc = write_poly(l_last, ext)) != CQ_OK || (rc = write_poly(pk->l_active_row, ext)) != CQ_OK) return rc;
  if ((rc = write_slice(pk->fixed_values, F, n)) != CQ_OK || (rc = write_slice(pk->fixed_polys, F, n)) != CQ_OK ||
      (rc = write_slice(pk->fixed_cosets, F, ext)) != CQ_OK)
    return rc;
  if ((rc = write_slice(pk->perm_values, PC, n)) != CQ_OK || (rc = write_slice(pk->perm_polys, PC, n)) != CQ_OK ||
      (rc = write_slice(pk->perm_cosets, PC, ext)) != CQ_OK)
    return rc;
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  *written = (size_t)(o - buf);
  return *written == total ? CQ_OK : c->fail(CQ_ERR_INTERNAL, "pk: serialized size mismatch");
}

int cq_pk_write_raw(cq_pk* pk, const uint8_t* selector_bits, uint32_t num_selectors, uint8_t* buf, size_t cap, size_t* written) {
  return pk_write_impl(pk, false, selector_bits, num_selectors, buf, cap, written);
}

int cq_pk_write(cq_pk* pk, int format, const uint8_t* selector_bits, uint32_t num_selectors, uint8_t* buf, size_t cap, size_t* written) {
  if (format != CQ_SERDE_PROCESSED && format != CQ_SERDE_RAW_BYTES && format != CQ_SERDE_RAW_BYTES_UNCHECKED)
    return pk ? pk->ctx->fail(CQ_ERR_ARG, "pk: unknown serde format") : CQ_ERR_ARG;
  return pk_write_impl(pk, format == CQ_SERDE_PROCESSED, selector_bits, num_selectors, buf, cap, written);
}

// MSM window tables of a sharded key: a rank only ever multiplies its slice of every (scalars, bases) range, so the
// 17 x SRS tables are built for those slices alone (the union of the slices over the MSMs that share an array: lengths
// n, n - 1, N, w N).  The whole-array tables of the SRS objects the key is built on are given up for that only while this
// key is their one user -- another key on the same params / table config keeps finding them, and the slices then resolve
// into them -- and are rebuilt when the key returns to world = 1 or is destroyed.
static int pk_shard_tables(cq_pk* pk) {
  cq_ctx* c = pk->ctx;
  for (auto& t : pk->shard_tables) msm_release_table(c, t.bases, t.n, t.c);
  pk->shard_tables.clear();
  if (!c->msm_precompute) return CQ_OK;
  const size_t n = (size_t)1 << pk->k, N = pk->table_cfg ? pk->table_cfg->N : 0;
  const bool has_cfg = pk->table_cfg && !pk->lookups.empty();
  int rc;
  if ((rc = pk_small_tables(pk)) != CQ_OK) return rc;  // the window width follows the length of a rank's point range
  if (pk->shard_world <= 1) {  // back to whole arrays
    if (pk->dropped_params_tables) {
      pk->dropped_params_tables = false;
      if ((rc = msm_register_tables(c, pk->params->g, n)) != CQ_OK || (rc = msm_register_tables(c, pk->params->g_lagrange, n)) != CQ_OK) return rc;
    }
    if (pk->dropped_cfg_tables) {
      pk->dropped_cfg_tables = false;
      if ((rc = msm_register_tables(c, pk->table_cfg->g1_lagrange, N)) != CQ_OK ||
          (rc = msm_register_tables(c, pk->table_cfg->g_lagrange_opening_at_0, N)) != CQ_OK)
        return rc;
    }
    return CQ_OK;
  }
  if (pk->params->key_users <= 1 && !pk->dropped_params_tables) {
    msm_unregister_tables(c, pk->params->g);
    msm_unregister_tables(c, pk->params->g_lagrange);
    pk->dropped_params_tables = true;
  }
  if (has_cfg && pk->table_cfg->key_users <= 1 && !pk->dropped_cfg_tables) {
    msm_unregister_tables(c, pk->table_cfg->g1_lagrange);
    msm_unregister_tables(c, pk->table_cfg->g_lagrange_opening_at_0);
    pk->dropped_cfg_tables = true;
  }
  struct Use { const G1Affine* b; size_t len; };
  std::vector<Use> uses{{pk->params->g_lagrange, n}, {pk->params->g, n}, {pk->params->g, n - 1}};
  if (has_cfg) {
    uses.push_back({pk->table_cfg->g1_lagrange, N});
    uses.push_back({pk->table_cfg->g_lagrange_opening_at_0, N});
  }
  if (pk->b0_g1_bound) uses.push_back({pk->b0_g1_bound, n - 1});
  // (the cached quotients [qs_0 | qs_1 | ...] are the key's own small arrays: their whole-array tables stay)
  std::vector<std::pair<const G1Affine*, const G1Affine*>> iv;
  for (auto& u : uses) {
    size_t lo, hi;
    shard_range(u.len, pk->shard_rank, pk->shard_world, lo, hi);
    if (hi > lo) iv.push_back({u.b + lo, u.b + hi});
  }
  std::sort(iv.begin(), iv.end());
  std::vector<std::pair<const G1Affine*, const G1Affine*>> merged;
  for (auto& x : iv) {
    if (!merged.empty() && x.first <= merged.back().second) merged.back().second = std::max(merged.back().second, x.second);
    else merged.push_back(x);
  }
  for (auto& m : merged) {
    bool held = false;
    const size_t len = (size_t)(m.second - m.first);
    if ((rc = msm_register_tables(c, m.first, len, pk->table_c, &held)) != CQ_OK) return rc;
    if (held) pk->shard_tables.push_back({m.first, len, pk->table_c});  // not held: served by a whole-array table that stayed
  }
  return CQ_OK;
}

int cq_pk_set_sharding(cq_pk* pk, uint32_t rank, uint32_t world, cq_allgather_fn fn, void* user) {
  if (!pk || world == 0 || rank >= world) return CQ_ERR_ARG;
  cq_ctx* c = pk->ctx;
  if (world > 1 && !fn && (!c->rccl_comm || c->rccl_world != world || c->rccl_rank != rank))
    return c->fail(CQ_ERR_ARG, "set_sharding: no all-gather callback and no matching RCCL communicator on the context");
  CQ_HIP(c, hipSetDevice(c->device));
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  pk->shard_rank = rank;
  pk->shard_world = world;
  // world = 1 over a one-rank RCCL communicator: still "sharded" -- every collective of the prover runs, over one rank
  pk->shard_single = world == 1 && !fn && c->rccl_comm && c->rccl_world == 1;
  pk->allgather = world > 1 ? fn : nullptr;
  pk->allgather_user = user;
  int rc = pk_shard_tables(pk);
  if (rc != CQ_OK) return rc;
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  return CQ_OK;
}

void cq_pk_destroy(cq_pk* pk) {
  if (!pk) return;
  hipStreamSynchronize(pk->ctx->stream);
  if (pk->domain) domain_destroy(pk->domain);
  if (pk->l_active_row) hipFree(pk->l_active_row);
  for (void* p : {(void*)pk->fixed_values, (void*)pk->fixed_polys, (void*)pk->fixed_cosets, (void*)pk->l0, (void*)pk->l_last,
                  (void*)pk->gate_prog, (void*)pk->constants, (void*)pk->lookup_prog, (void*)pk->legacy_prog, (void*)pk->perm_values, (void*)pk->perm_polys, (void*)pk->perm_cosets,
                  (void*)pk->omega_powers, (void*)pk->ext_pow_lo, (void*)pk->ext_pow_hi})
    if (p) hipFree(p);
  // window tables: the slices of a sharded key go, the whole-array tables it had given up come back (their owners --
  // params, table config -- are still alive: a key never outlives them), its references are returned
  if (pk->shard_world > 1 || pk->dropped_params_tables || pk->dropped_cfg_tables) {
    pk->shard_world = 1;
    (void)pk_shard_tables(pk);
  }
  for (auto& t : pk->held_tables) msm_release_table(pk->ctx, t.bases, t.n, t.c);
  for (int q = 0; q < 2; q++)
    if (pk->b_row_bases[q]) hipFree(pk->b_row_bases[q]);
  if (pk->own_b0 && pk->b0_g1_bound) {
    msm_unregister_tables(pk->ctx, pk->b0_g1_bound);
    hipFree(pk->b0_g1_bound);
  }
  for (auto p : pk->qs_concat) {
    msm_unregister_tables(pk->ctx, p);
    hipFree(p);
  }
  if (pk->counted_users) {
    cq_params* params = pk->params;
    cq_table_config* cfg = pk->table_cfg;
    if (--params->key_users == 0 && params->owner_released) cq_params_destroy(params);
    if (cfg && --cfg->key_users == 0 && cfg->owner_released) cq_table_config_destroy(cfg);
  }
  delete pk;
}

}  // extern "C"

// C ABI: CQ table objects, create_proof and the proving-key accessors around it, SHA witness fill and tables, harness RNGs.
// (The proving key itself is built, serialized and destroyed in pk.hip.)
#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "assigned_host.hpp"
#include "building.hpp"
#include "cq.hpp"
#include "xoshiro.hpp"
#include "ctx.hpp"
#include "g1fft.hpp"
#include "plonk.hpp"
#include "poly.hpp"
#include "prover.hpp"
#include "setup.hpp"
#include "msm.hpp"
#include "comm.hpp"
#include "serde.hpp"

using namespace cq;

static bool is_pow2(size_t x) { return x && !(x & (x - 1)); }
static uint32_t log2u(size_t x) {
  uint32_t l = 0;
  while (((size_t)1 << (l + 1)) <= x) l++;
  return l;
}

extern "C" {

// ---- StaticTableConfig ---------------------------------------------------------------------------
// Shared by the constructors: the object `t` (already under its Building guard) gets its two arrays ...
static int table_config_alloc(cq_ctx* c, size_t size, cq_table_config* t, cq_table_config** out) {
  *out = nullptr;
  t->ctx = c;
  t->N = size;
  t->log_n = log2u(size);
  CQ_HIP(c, hipSetDevice(c->device));
  int rc = c->dev_alloc(&t->g1_lagrange, size, "table config");
  return rc != CQ_OK ? rc : c->dev_alloc(&t->g_lagrange_opening_at_0, size, "table config");
}
// ... and, once they are filled, their window tables
static int table_config_finish(Building<cq_table_config>& guard, cq_table_config** out) {
  cq_ctx* c = guard.c;
  int rc;
  if (c->msm_precompute && ((rc = msm_register_tables(c, guard.p->g1_lagrange, guard.p->N)) != CQ_OK ||
                            (rc = msm_register_tables(c, guard.p->g_lagrange_opening_at_0, guard.p->N)) != CQ_OK))
    return rc;
  return guard.finish(out);
}

int cq_table_config_create(cq_ctx* c, size_t size, const uint64_t* g1_lagrange, const uint64_t* opening_at_0,
                           cq_table_config** out) {
  if (!c || !g1_lagrange || !opening_at_0 || !out || !is_pow2(size) || size > (1u << 28)) return CQ_ERR_ARG;
  Building<cq_table_config> guard(new cq_table_config(), cq_table_config_destroy, c);
  cq_table_config* t = guard.p;
  int rc = table_config_alloc(c, size, t, out);
  if (rc != CQ_OK) return rc;
  const size_t bytes = size * sizeof(G1Affine);
  CQ_HIP(c, hipMemcpyAsync(t->g1_lagrange, g1_lagrange, bytes, hipMemcpyHostToDevice, c->stream));
  CQ_HIP(c, hipMemcpyAsync(t->g_lagrange_opening_at_0, opening_at_0, bytes, hipMemcpyHostToDevice, c->stream));
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  return table_config_finish(guard, out);
}

int cq_table_config_setup_from_toxic_waste(cq_ctx* c, size_t size, const uint64_t s[4], cq_table_config** out) {
  if (!c || !s || !out || !is_pow2(size) || size > (1u << 28)) return CQ_ERR_ARG;
  Building<cq_table_config> guard(new cq_table_config(), cq_table_config_destroy, c);
  cq_table_config* t = guard.p;
  int rc = table_config_alloc(c, size, t, out);
  if (rc != CQ_OK) return rc;
  void* tmp;
  if ((rc = c->ensure_scratch(Scratch::EntryA, 2 * size * sizeof(Fr), &tmp)) != CQ_OK) return rc;
  Fr* lag_sc = (Fr*)tmp;
  Fr* tmp_sc = lag_sc + size;
  const Fr sf = Fr::from_limbs64(s);
  if ((rc = srs_powers_and_lagrange(c, t->log_n, sf, nullptr, t->g1_lagrange, tmp_sc, lag_sc)) != CQ_OK) return rc;
  if ((rc = srs_opening_at_zero(c, t->log_n, sf, lag_sc, tmp_sc, t->g_lagrange_opening_at_0)) != CQ_OK) return rc;
  return table_config_finish(guard, out);
}

// StaticTableConfig from the powers: both arrays are inverse G1 FFTs of them (kzg/commitment.rs:125-170)
int cq_table_config_from_srs(cq_ctx* c, size_t size, const uint64_t* srs_g1, size_t srs_len, int on_device, cq_table_config** out) {
  if (!c || !srs_g1 || !out || !is_pow2(size) || size > (1u << 28) || srs_len < size) return CQ_ERR_ARG;
  Building<cq_table_config> guard(new cq_table_config(), cq_table_config_destroy, c);
  cq_table_config* t = guard.p;
  int rc = table_config_alloc(c, size, t, out);
  if (rc != CQ_OK) return rc;
  const G1Affine* srs = (const G1Affine*)srs_g1;
  if (!on_device) {
    G1Affine* up = nullptr;
    if ((rc = guard.temp(&up, size, "table config srs")) != CQ_OK) return rc;
    CQ_HIP(c, hipMemcpyAsync(up, srs_g1, size * sizeof(G1Affine), hipMemcpyHostToDevice, c->stream));
    srs = up;
  }
  // [L_i(s)] = (1/N) sum_j w^(-ij) [s^j]
  if ((rc = g1_to_lagrange(c, srs, t->log_n, t->g1_lagrange, true)) != CQ_OK) return rc;
  // [(L_i(s) - L_i(0)) / s]: L_i(X) = (1/N) sum_m w^(-im) X^m and L_i(0) = 1/N, so the quotient is
  // (1/N) sum_(m>=1) w^(-im) X^(m-1) -- power j = m - 1 < N - 1 sits at place j + 1 of the transform's input
  if ((rc = g1_to_lagrange_shifted(c, srs, (uint32_t)(size - 1), 1, t->log_n, t->g_lagrange_opening_at_0, true)) != CQ_OK) return rc;
  return table_config_finish(guard, out);
}

void cq_table_config_destroy(cq_table_config* t) {
  if (!t) return;
  if (t->key_users > 0) {  // a key still uses it: the last one frees it (see cq_params_destroy)
    t->owner_released = true;
    return;
  }
  hipStreamSynchronize(t->ctx->stream);
  msm_unregister_tables(t->ctx, t->g1_lagrange);
  msm_unregister_tables(t->ctx, t->g_lagrange_opening_at_0);
  if (t->g1_lagrange) hipFree(t->g1_lagrange);
  if (t->g_lagrange_opening_at_0) hipFree(t->g_lagrange_opening_at_0);
  delete t;
}

int cq_table_config_download(cq_table_config* t, uint64_t* g1_lagrange, uint64_t* opening_at_0) {
  if (!t) return CQ_ERR_ARG;
  cq_ctx* c = t->ctx;
  const size_t bytes = t->N * sizeof(G1Affine);
  if (g1_lagrange) CQ_HIP(c, hipMemcpyAsync(g1_lagrange, t->g1_lagrange, bytes, hipMemcpyDeviceToHost, c->stream));
  if (opening_at_0) CQ_HIP(c, hipMemcpyAsync(opening_at_0, t->g_lagrange_opening_at_0, bytes, hipMemcpyDeviceToHost, c->stream));
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  return CQ_OK;
}

// ---- StaticTableValues -----------------------------------------------------------------------------
// Shared by the constructors, after their argument check: the object `t` (already under its Building guard) gets its arrays,
// the values and their index; nothing to undo here on failure
static int table_alloc(cq_ctx* c, size_t size, const uint64_t* values, cq_static_table* t, cq_static_table** out) {
  *out = nullptr;
  t->ctx = c;
  t->N = size;
  CQ_HIP(c, hipSetDevice(c->device));
  int rc;
  if ((rc = c->dev_alloc(&t->values, size, "static table")) != CQ_OK || (rc = c->dev_alloc(&t->qs, size, "static table")) != CQ_OK) return rc;
  CQ_HIP(c, hipMemcpyAsync(t->values, values, size * sizeof(Fr), hipMemcpyHostToDevice, c->stream));
  return cq_table_build_index(c, t->values, (uint32_t)size, &t->slots, &t->nslots);
}
int cq_static_table_create(cq_ctx* c, size_t size, const uint64_t* values, const uint64_t* qs_affine, cq_static_table** out) {
  if (!c || !values || !qs_affine || !out || !is_pow2(size) || size > (1u << 28)) return CQ_ERR_ARG;  // static_lookup.rs:80
  Building<cq_static_table> guard(new cq_static_table(), cq_static_table_destroy, c);
  cq_static_table* t = guard.p;
  int rc = table_alloc(c, size, values, t, out);
  if (rc != CQ_OK) return rc;
  CQ_HIP(c, hipMemcpyAsync(t->qs, qs_affine, size * sizeof(G1Affine), hipMemcpyHostToDevice, c->stream));
  return guard.finish(out);
}

int cq_static_table_setup_from_toxic_waste(cq_ctx* c, size_t size, const uint64_t* values, const uint64_t s[4],
                                           cq_static_table** out) {
  if (!c || !values || !s || !out || !is_pow2(size) || size > (1u << 28)) return CQ_ERR_ARG;
  Building<cq_static_table> guard(new cq_static_table(), cq_static_table_destroy, c);
  cq_static_table* t = guard.p;
  int rc = table_alloc(c, size, values, t, out);
  if (rc != CQ_OK) return rc;
  // T(s): interpolate the values over the size-N domain, evaluate at s
  if ((rc = domain_create(c, 2, log2u(size), &guard.dom)) != CQ_OK) return rc;
  cq_domain* dom = guard.dom;
  void* tmp;
  if ((rc = c->ensure_scratch(Scratch::EntryA, 2 * size * sizeof(Fr), &tmp)) != CQ_OK) return rc;
  Fr* coeffs = (Fr*)tmp;
  Fr* sc = coeffs + size;
  const Fr sf = Fr::from_limbs64(s);
  Fr ts;
  if ((rc = domain_lagrange_to_coeff(dom, t->values, coeffs, 1, size, size)) != CQ_OK) return rc;
  if ((rc = poly_eval(c, coeffs, (uint32_t)size, sf, &ts)) != CQ_OK) return rc;
  if ((rc = cq_qs_scalars(c, t->values, (uint32_t)size, ts, sf, dom->omega, dom->ifft_divisor, sc)) != CQ_OK) return rc;
  if ((rc = fixed_base_mul(c, sc, (uint32_t)size, t->qs)) != CQ_OK) return rc;
  return guard.finish(out);
}

void cq_static_table_destroy(cq_static_table* t) {
  if (!t) return;
  hipStreamSynchronize(t->ctx->stream);
  if (t->values) hipFree(t->values);
  if (t->qs) hipFree(t->qs);
  if (t->slots) hipFree(t->slots);
  delete t;
}

int cq_static_table_download_qs(cq_static_table* t, uint64_t* qs_affine) {
  if (!t || !qs_affine) return CQ_ERR_ARG;
  cq_ctx* c = t->ctx;
  CQ_HIP(c, hipMemcpyAsync(qs_affine, t->qs, t->N * sizeof(G1Affine), hipMemcpyDeviceToHost, c->stream));
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  return CQ_OK;
}

// ---- proving key: everything that is not construction, serialization or sharding (pk.hip) ------------
int cq_pk_set_opener(cq_pk* pk, int opener) {
  if (!pk || (opener != CQ_OPENER_GWC && opener != CQ_OPENER_SHPLONK)) return CQ_ERR_ARG;
  pk->opener = opener;
  return CQ_OK;
}

int cq_pk_set_rng_fill(cq_pk* pk, cq_rng_fill_fn fill) {
  if (!pk) return CQ_ERR_ARG;
  pk->rng_fill = fill;
  return CQ_OK;
}

int cq_pk_set_column_sharding(cq_pk* pk, int on, cq_bcast_fn fn, void* user) {
  if (!pk) return CQ_ERR_ARG;
  pk->shard_columns = on != 0;
  pk->bcast = fn;
  pk->bcast_user = user;
  return CQ_OK;
}

int cq_pk_set_resident_sharding(cq_pk* pk, int on, cq_exchange_fn fn, void* user) {
  if (!pk) return CQ_ERR_ARG;
  pk->shard_resident = on != 0;
  pk->exchange = fn;
  pk->exchange_user = user;
  return CQ_OK;
}

uint32_t cq_pk_usable_rows(const cq_pk* pk) { return pk ? pk->u : 0; }
const uint64_t* cq_pk_b_row_bases_dev(const cq_pk* pk, int which) {
  return pk && (which == 0 || which == 1) ? (const uint64_t*)pk->b_row_bases[which] : nullptr;
}

size_t cq_pk_proof_size(const cq_pk* pk) {
  if (!pk) return 0;
  const size_t L = pk->lookups.size(), S = pk->perm_sets();
  // one opening witness per distinct evaluation point (gwc/prover.rs:42-91)
  const size_t PL = pk->legacy.size();
  const size_t openings = pk->opener == CQ_OPENER_SHPLONK ? 2 : pk->opening_rotations().size();
  const size_t points = pk->num_advice + 2 * L + 3 * PL + S + 5 * L + 1 + pk->domain->quotient_poly_degree + openings;
  const size_t scalars = pk->advice_queries.size() + pk->fixed_queries.size() + 1 + pk->perm_columns.size() + (S ? 3 * S - 1 : 0) + 3 * L + 5 * PL;
  return 32 * (points + scalars);
}

static int create_proof_any(cq_pk* pk, const uint64_t* const* advice_dev, const uint64_t* const* instances,
                            const size_t* instance_lens, cq_rng_next_u64 rng, void* rng_state, uint8_t* proof,
                            size_t proof_cap, size_t* proof_len, cq_phase_fn phase_fn = nullptr, void* phase_user = nullptr) {
  if (!pk || (!advice_dev && pk->num_advice) || !rng || !proof || !proof_len) return CQ_ERR_ARG;
  cq_ctx* c = pk->ctx;
  // "InvalidInstances" (prover.rs:73-82)
  if (pk->num_instance && (!instances || !instance_lens)) return c->fail(CQ_ERR_ARG, "create_proof: instance columns missing");
  CQ_HIP(c, hipSetDevice(c->device));
  std::vector<uint8_t> out;
  if (pk->num_phases > 1 && !phase_fn) return c->fail(CQ_ERR_ARG, "create_proof: a multi-phase circuit needs cq_create_proof_phases");
  // `overrun` counts the words THIS proof asked for beyond the stream (a caller's struct may hold anything there)
  if (rng == cq_buffer_rng_next_u64) ((cq_buffer_rng*)rng_state)->overrun = 0;
  int rc = create_proof_dev(pk, advice_dev, instances, instance_lens, phase_fn, phase_user, rng, rng_state, out);
  // A sharded proof that fails on this rank (over RCCL) leaves its peers in, or heading for, a collective this rank will not
  // join: give up the communicator, so that they fail too (asynchronous error or their wait's time-out) instead of
  // hanging.  Not for the failures every rank runs into alike, at the same point of the same program, with nothing pending
  // between them -- a witness value missing from a table, an identity commitment, a bad argument: those just return.
  const bool rank_local = rc == CQ_ERR_HIP || rc == CQ_ERR_INTERNAL || rc == CQ_ERR_NO_DEVICE;
  if (rank_local && pk->sharded() && !pk->allgather && c->rccl_comm && !pk->shard_single) {
    const std::string keep = c->err;
    cq::comm_rccl_abort(c);
    c->err = keep + " (sharded proof: this rank's RCCL communicator was aborted so that its peers do not hang)";
  }
  // An exhausted stream reads as zeros: the proof would not be zero-knowledge, and an all-zero random polynomial also
  // trips the transcript's identity-commitment check -- both are reported as what they are.  Any other error keeps its code.
  if (rng == cq_buffer_rng_next_u64 && ((cq_buffer_rng*)rng_state)->overrun && (rc == CQ_OK || rc == CQ_ERR_TRANSCRIPT))
    return c->fail(CQ_ERR_ARG, "create_proof: the pre-drawn RNG stream ran out (blinding would be zero)");
  if (rc != CQ_OK) return rc;
  if (out.size() > proof_cap) return c->fail(CQ_ERR_ARG, "proof buffer too small");
  memcpy(proof, out.data(), out.size());
  *proof_len = out.size();
  return CQ_OK;
}

int cq_create_proof(cq_pk* pk, const uint64_t* const* advice_dev, cq_rng_next_u64 rng, void* rng_state, uint8_t* proof,
                    size_t proof_cap, size_t* proof_len) {
  return create_proof_any(pk, advice_dev, nullptr, nullptr, rng, rng_state, proof, proof_cap, proof_len);
}

static int create_proof_host_any(cq_pk* pk, const uint64_t* const* advice, const uint64_t* const* instances,
                                 const size_t* instance_lens, cq_rng_next_u64 rng, void* rng_state, uint8_t* proof,
                                 size_t proof_cap, size_t* proof_len) {
  if (!pk || (!advice && pk->num_advice)) return CQ_ERR_ARG;
  cq_ctx* c = pk->ctx;
  CQ_HIP(c, hipSetDevice(c->device));
  const size_t n = (size_t)1 << pk->k;
  void* stage;
  int rc;
  if ((rc = c->ensure_scratch(Scratch::HostAdvice, (size_t)pk->num_advice * n * sizeof(Fr) + 64, &stage)) != CQ_OK) return rc;
  std::vector<const uint64_t*> ptrs(pk->num_advice);
  for (uint32_t a = 0; a < pk->num_advice; a++) {
    Fr* d = (Fr*)stage + (size_t)a * n;
    CQ_HIP(c, hipMemcpyAsync(d, advice[a], (size_t)pk->u * sizeof(Fr), hipMemcpyHostToDevice, c->stream));
    ptrs[a] = (const uint64_t*)d;
  }
  return create_proof_any(pk, ptrs.data(), instances, instance_lens, rng, rng_state, proof, proof_cap, proof_len);
}

// create_proof from the WitnessCollection hand-over (prover.rs:337-360): the advice columns still hold Assigned cells and
// batch_invert_assigned (poly.rs:212-241) runs first.  Numerators go up as create_proof_host_any uploads columns, the
// sparse denominators into a buffer of their own, and the columns are resolved in place on the proof's stream.  Entries
// that name a blinding row are dropped here: those cells are overwritten with blinding (prover.rs:346-349).
int cq_create_proof_assigned(cq_pk* pk, const cq_assigned_column* cols, const uint64_t* const* instances, const size_t* instance_lens,
                             cq_rng_next_u64 rng, void* rng_state, uint8_t* proof, size_t proof_cap, size_t* proof_len) {
  if (!pk || (!cols && pk->num_advice)) return CQ_ERR_ARG;
  cq_ctx* c = pk->ctx;
  if (pk->num_phases > 1)
    return c->fail(CQ_ERR_ARG, "create_proof_assigned: multi-phase circuits are not covered (the phase callback of cq_create_proof_phases writes device columns)");
  CQ_HIP(c, hipSetDevice(c->device));
  const size_t n = (size_t)1 << pk->k, A = pk->num_advice;
  std::vector<uint32_t> off(A + 1, 0);
  for (size_t a = 0; a < A; a++) {
    const cq_assigned_column& col = cols[a];
    if (!col.num || (col.den_count && (!col.den_rows || !col.den)))
      return c->fail(CQ_ERR_ARG, "create_proof_assigned: column " + std::to_string(a) + ": null array");
    const size_t bad = assigned_rows_first_bad(col.den_rows, col.den_count, n);
    if (bad != col.den_count)
      return c->fail(CQ_ERR_ARG, "create_proof_assigned: column " + std::to_string(a) + ", entry " + std::to_string(bad) + ": row " +
                                     std::to_string(col.den_rows[bad]) + " is not below n or does not ascend");
    const size_t kept = assigned_rows_below(col.den_rows, col.den_count, pk->u);
    if ((uint64_t)off[a] + kept > 0x7fffffffull) return c->fail(CQ_ERR_ARG, "create_proof_assigned: too many rational cells");
    off[a + 1] = off[a] + (uint32_t)kept;
  }
  void *stage, *sparse;
  int rc;
  if ((rc = c->ensure_scratch(Scratch::HostAdvice, A * n * sizeof(Fr) + 64, &stage)) != CQ_OK) return rc;
  const size_t total = off[A], rows_bytes = (total * sizeof(uint32_t) + 31) & ~(size_t)31;
  if ((rc = c->ensure_scratch(Scratch::AssignedDen, rows_bytes + 2 * total * sizeof(Fr) + 64, &sparse)) != CQ_OK) return rc;
  uint32_t* rows = (uint32_t*)sparse;
  Fr* den = (Fr*)((char*)sparse + rows_bytes);
  Fr* work = den + total;
  std::vector<const uint64_t*> ptrs(A);
  std::vector<Fr*> out(A);
  for (size_t a = 0; a < A; a++) {
    out[a] = (Fr*)stage + a * n;
    ptrs[a] = (const uint64_t*)out[a];
    CQ_HIP(c, hipMemcpyAsync(out[a], cols[a].num, (size_t)pk->u * sizeof(Fr), hipMemcpyHostToDevice, c->stream));
    const size_t cnt = off[a + 1] - off[a];
    if (!cnt) continue;
    CQ_HIP(c, hipMemcpyAsync(rows + off[a], cols[a].den_rows, cnt * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    CQ_HIP(c, hipMemcpyAsync(den + off[a], cols[a].den, cnt * sizeof(Fr), hipMemcpyHostToDevice, c->stream));
  }
  if ((rc = poly_resolve_assigned(c, (const Fr* const*)out.data(), out.data(), off.data(), (uint32_t)A, rows, den, pk->u, work, nullptr)) != CQ_OK)
    return rc;
  return create_proof_any(pk, ptrs.data(), instances, instance_lens, rng, rng_state, proof, proof_cap, proof_len);
}

int cq_create_proof_host(cq_pk* pk, const uint64_t* const* advice, cq_rng_next_u64 rng, void* rng_state, uint8_t* proof,
                         size_t proof_cap, size_t* proof_len) {
  return create_proof_host_any(pk, advice, nullptr, nullptr, rng, rng_state, proof, proof_cap, proof_len);
}

int cq_create_proof_phases(cq_pk* pk, uint64_t* const* advice_dev, const uint64_t* const* instances, const size_t* instance_lens,
                           cq_phase_fn phase_fn, void* phase_user, cq_rng_next_u64 rng, void* rng_state, uint8_t* proof,
                           size_t proof_cap, size_t* proof_len) {
  return create_proof_any(pk, advice_dev, instances, instance_lens, rng, rng_state, proof, proof_cap, proof_len, phase_fn, phase_user);
}

int cq_create_proof_instances(cq_pk* pk, const uint64_t* const* advice, int advice_on_device, const uint64_t* const* instances,
                              const size_t* instance_lens, cq_rng_next_u64 rng, void* rng_state, uint8_t* proof,
                              size_t proof_cap, size_t* proof_len) {
  return advice_on_device ? create_proof_any(pk, advice, instances, instance_lens, rng, rng_state, proof, proof_cap, proof_len)
                          : create_proof_host_any(pk, advice, instances, instance_lens, rng, rng_state, proof, proof_cap, proof_len);
}

// Several instances of one circuit (independent witnesses, independent transcripts and RNG streams; the reference's
// `circuits: &[ConcreteCircuit]`, plonk/prover.rs:419-463, proves them under ONE transcript and asserts a single circuit,
// :413-417, so a batch here means independent proofs).  The proofs run on `lanes` contexts of their own on the same GPU,
// one host thread each: while one proof sits in the latency-bound tail of an MSM launch or waits for its host (transcript,
// normalisation), the others' kernels fill the chip -- BASELINE configs[4].  Byte for byte the proofs cq_create_proof
// gives one at a time.
int cq_create_proof_batch(cq_pk* pk, size_t count, const uint64_t* const* const* advice_dev, cq_rng_next_u64 rng,
                          void* const* rng_states, uint8_t* const* proofs, size_t proof_cap, size_t* proof_lens, uint32_t lanes) {
  if (!pk || (count && (!advice_dev || !rng || !rng_states || !proofs || !proof_lens))) return CQ_ERR_ARG;
  cq_ctx* c = pk->ctx;
  if (pk->num_instance || pk->num_phases > 1) return c->fail(CQ_ERR_ARG, "create_proof_batch: circuits with instance columns or several phases go through cq_create_proof_instances / _phases");
  if (pk->sharded()) return c->fail(CQ_ERR_ARG, "create_proof_batch: the key is sharded across ranks");
  if (!count) return CQ_OK;
  CQ_HIP(c, hipSetDevice(c->device));
  if (lanes == 0) lanes = 3;
  lanes = (uint32_t)std::min<size_t>(lanes, count);
  while (c->lanes.size() < lanes) {
    cq_ctx* lane = nullptr;
    int rc = cq_ctx_create(c->device, nullptr, &lane);
    if (rc != CQ_OK) return c->fail(rc, "create_proof_batch: lane context");
    lane->parent = c;
    c->lanes.push_back(lane);
  }
  CQ_HIP(c, hipStreamSynchronize(c->stream));  // whatever filled the witnesses on the caller's stream is done
  (void)c->pool();  // the lanes share the parent's worker threads: created here, before several threads would race to
  std::atomic<size_t> next{0};
  std::atomic<int> first_rc{CQ_OK};
  std::mutex err_mu;
  std::string err;
  auto worker = [&](uint32_t li) {
    cq_ctx* lc = c->lanes[li];
    if (hipSetDevice(lc->device) != hipSuccess) {
      first_rc.store(CQ_ERR_HIP);
      return;
    }
    // the key as this lane sees it: same device data, this lane's context (stream, scratch, twiddle cache)
    cq_pk lane_pk = *pk;
    cq_domain lane_dom = *pk->domain;
    lane_dom.ctx = lc;
    lane_pk.ctx = lc;
    lane_pk.domain = &lane_dom;
    for (;;) {
      const size_t i = next.fetch_add(1);
      if (i >= count || first_rc.load() != CQ_OK) break;
      std::vector<uint8_t> out;
      if (rng == cq_buffer_rng_next_u64) ((cq_buffer_rng*)rng_states[i])->overrun = 0;
      int rc = create_proof_dev(&lane_pk, advice_dev[i], nullptr, nullptr, nullptr, nullptr, rng, rng_states[i], out);
      if ((rc == CQ_OK || rc == CQ_ERR_TRANSCRIPT) && rng == cq_buffer_rng_next_u64 && ((cq_buffer_rng*)rng_states[i])->overrun) {
        rc = CQ_ERR_ARG;
        lc->err = "create_proof: the pre-drawn RNG stream ran out (blinding would be zero)";
      }
      if (rc == CQ_OK && out.size() > proof_cap) {
        rc = CQ_ERR_ARG;
        lc->err = "proof buffer too small";
      }
      if (rc != CQ_OK) {
        std::lock_guard<std::mutex> lk(err_mu);
        if (first_rc.load() == CQ_OK) {
          first_rc.store(rc);
          err = "proof " + std::to_string(i) + ": " + lc->err;
        }
        break;
      }
      memcpy(proofs[i], out.data(), out.size());
      proof_lens[i] = out.size();
    }
    hipStreamSynchronize(lc->stream);
  };
  std::vector<std::thread> th;
  for (uint32_t li = 1; li < lanes; li++) {
    try {
      th.emplace_back(worker, li);
    } catch (...) {  // no thread to be had: the remaining lanes' share falls to the ones that run
      break;
    }
  }
  worker(0);
  for (auto& t : th) t.join();
  if (first_rc.load() != CQ_OK) return c->fail(first_rc.load(), err);
  return CQ_OK;
}

// fixed_commitments (keygen.rs:247-250) and permutation::VerifyingKey::commitments (permutation/keygen.rs:115-149)
int cq_pk_vk_commitments(cq_pk* pk, uint64_t* fixed_commitments, uint64_t* permutation_commitments) {
  if (!pk) return CQ_ERR_ARG;
  cq_ctx* c = pk->ctx;
  CQ_HIP(c, hipSetDevice(c->device));
  const size_t n = (size_t)1 << pk->k;
  for (int which = 0; which < 2; which++) {
    const size_t cnt = which ? pk->perm_columns.size() : pk->num_fixed;
    uint64_t* dst = which ? permutation_commitments : fixed_commitments;
    const Fr* src = which ? pk->perm_values : pk->fixed_values;
    if (!cnt) continue;
    if (!dst) return c->fail(CQ_ERR_ARG, "vk commitments: null output");
    for (size_t i = 0; i < cnt; i++) {
      uint64_t jac[12];
      int rc = cq_commit_lagrange_dev(pk->params, (const uint64_t*)(src + i * n), n, jac);
      if (rc != CQ_OK) return rc;
      if ((rc = cq_g1_to_affine(jac, dst + 8 * i)) != CQ_OK) return rc;
    }
  }
  return CQ_OK;
}

// ---- SHA witness fill --------------------------------------------------------------------------------
int cq_sha_witness_fill_dev(cq_ctx* c, const uint32_t* words_dev, size_t nwords, uint32_t pairs, size_t n,
                            uint64_t* const* cols_dev) {
  if (!c || !words_dev || !cols_dev || pairs == 0 || pairs > 8 || nwords > 0x3fffffffull || n > 0x7fffffffull) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  ShaCols sc;
  for (uint32_t i = 0; i < 16; i++) sc.p[i] = i < 2 * pairs ? (Fr*)cols_dev[i] : nullptr;
  return sha_witness_fill(c, words_dev, (uint32_t)nwords, pairs, (uint32_t)n, sc);
}

int cq_sha_spread_table_dev(cq_ctx* c, size_t size, uint64_t* dense_dev, uint64_t* spread_dev) {
  if (!c || !dense_dev || !spread_dev || size == 0 || size > 65536) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  return sha_spread_table(c, (uint32_t)size, (Fr*)dense_dev, (Fr*)spread_dev);
}

// ---- sha/src/tables.rs generators ----------------------------------------------------------------------
int cq_sha_synthesis_table_dev(cq_ctx* c, int kind, uint32_t first_limb_len, uint32_t second_limb_len, uint64_t* out_dev) {
  if (!c || !out_dev || kind < 0 || kind > 3 || first_limb_len == 0 || second_limb_len == 0 ||
      first_limb_len + 2 * second_limb_len > 28)
    return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  return sha_synthesis_table(c, (uint32_t)kind, first_limb_len, second_limb_len, out_dev);
}
int cq_sha_decomposition_table_dev(cq_ctx* c, uint32_t first_limb_len, uint32_t second_limb_len, uint32_t k_bits,
                                   uint64_t* out_dev) {
  if (!c || !out_dev || k_bits > 28 || first_limb_len == 0 || second_limb_len == 0) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  return sha_decomposition_table(c, first_limb_len, second_limb_len, k_bits, out_dev);
}

// ---- StaticTableValues::new (static_lookup.rs:78-126): the reference's O(N^2) construction on the GPU ----
int cq_static_table_new(cq_ctx* c, size_t size, const uint64_t* values, const uint64_t* srs_g1, cq_static_table** out) {
  if (!c || !values || !srs_g1 || !out || !is_pow2(size) || size > (1u << 20)) return CQ_ERR_ARG;
  Building<cq_static_table> guard(new cq_static_table(), cq_static_table_destroy, c);
  cq_static_table* t = guard.p;
  int rc = table_alloc(c, size, values, t, out);
  if (rc != CQ_OK) return rc;
  const uint32_t N = (uint32_t)size;
  if ((rc = domain_create(c, 2, log2u(size), &guard.dom)) != CQ_OK) return rc;
  cq_domain* dom = guard.dom;
  const uint32_t group = 16;  // roots per MSM launch
  G1Affine* srs = nullptr;
  Fr *coeffs = nullptr, *quot = nullptr;
  if ((rc = guard.temp(&srs, size, "static_table_new")) != CQ_OK || (rc = guard.temp(&coeffs, size, "static_table_new")) != CQ_OK ||
      (rc = guard.temp(&quot, (size_t)group * size, "static_table_new")) != CQ_OK)
    return rc;
  CQ_HIP(c, hipMemcpyAsync(srs, srs_g1, size * sizeof(G1Affine), hipMemcpyHostToDevice, c->stream));
  guard.reg.push_back(srs);  // unregistering an array that never got tables is a no-op
  if (c->msm_precompute && (rc = msm_register_tables(c, srs, size)) != CQ_OK) return rc;
  if ((rc = domain_lagrange_to_coeff(dom, t->values, coeffs, 1, size, size)) != CQ_OK) return rc;  // :99-105
  std::vector<uint64_t> jac(group * 12);
  std::vector<G1Affine> host_qs(size);
  for (uint32_t first = 0; first < N; first += group) {
    const uint32_t cnt = std::min(group, N - first);
    if ((rc = cq_table_quotients(c, coeffs, N, dom->omega, dom->ifft_divisor, first, cnt, quot)) != CQ_OK) return rc;  // :111-115
    std::vector<const Fr*> sc(cnt);
    std::vector<const G1Affine*> bs(cnt, srs);
    for (uint32_t r = 0; r < cnt; r++) sc[r] = quot + (size_t)r * N;
    if ((rc = cq_msm_multi(c, sc.data(), bs.data(), N - 1, cnt, jac.data())) != CQ_OK) return rc;  // :117
    for (uint32_t r = 0; r < cnt; r++) {
      G1Jac q = {Fq::from_limbs64(jac.data() + 12 * r), Fq::from_limbs64(jac.data() + 12 * r + 4),
                 Fq::from_limbs64(jac.data() + 12 * r + 8)};
      host_qs[first + r] = jac_to_affine(q);
    }
  }
  CQ_HIP(c, hipMemcpyAsync(t->qs, host_qs.data(), size * sizeof(G1Affine), hipMemcpyHostToDevice, c->stream));
  return guard.finish(out);
}

static int static_table_new_fk(cq_ctx* c, size_t size, const uint64_t* values, const uint64_t* srs_g1, bool srs_on_device,
                               cq_static_table** out) {
  if (!c || !values || !srs_g1 || !out || !is_pow2(size) || size < 2 || size > (1u << 22)) return CQ_ERR_ARG;
  Building<cq_static_table> guard(new cq_static_table(), cq_static_table_destroy, c);
  cq_static_table* t = guard.p;
  int rc = table_alloc(c, size, values, t, out);
  if (rc != CQ_OK) return rc;
  if ((rc = domain_create(c, 2, log2u(size), &guard.dom)) != CQ_OK) return rc;
  G1Affine* srs = nullptr;
  Fr* coeffs = nullptr;
  if ((!srs_on_device && (rc = guard.temp(&srs, size, "static_table_new_fk")) != CQ_OK) || (rc = guard.temp(&coeffs, size, "static_table_new_fk")) != CQ_OK)
    return rc;
  if (!srs_on_device) CQ_HIP(c, hipMemcpyAsync(srs, srs_g1, size * sizeof(G1Affine), hipMemcpyHostToDevice, c->stream));
  if ((rc = domain_lagrange_to_coeff(guard.dom, t->values, coeffs, 1, size, size)) != CQ_OK) return rc;  // :99-105
  // resident powers belong to the trapdoor-free setup path and take its FFT; the quotients are the same bytes either way
  if ((rc = fk_table_quotients(c, coeffs, srs_on_device ? (const G1Affine*)srs_g1 : srs, log2u(size), t->qs, srs_on_device)) != CQ_OK) return rc;
  return guard.finish(out);
}
int cq_static_table_new_fk(cq_ctx* c, size_t size, const uint64_t* values, const uint64_t* srs_g1, cq_static_table** out) {
  return static_table_new_fk(c, size, values, srs_g1, false, out);
}
int cq_static_table_new_fk_dev(cq_ctx* c, size_t size, const uint64_t* values, const uint64_t* srs_g1_dev, cq_static_table** out) {
  return static_table_new_fk(c, size, values, srs_g1_dev, true, out);
}

// ---- harness RNGs ----------------------------------------------------------------------------------------
void cq_xoshiro256ss_seed(uint64_t seed, uint64_t state[4]) {
  uint64_t z = seed;
  for (int i = 0; i < 4; i++) {  // splitmix64
    z += 0x9E3779B97F4A7C15ull;
    uint64_t x = z;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    state[i] = x ^ (x >> 31);
  }
}
static inline uint64_t rotl64(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
uint64_t cq_xoshiro256ss_next_u64(void* st) {
  uint64_t* s = (uint64_t*)st;
  const uint64_t result = rotl64(s[1] * 5, 7) * 9;
  const uint64_t t = s[1] << 17;
  s[2] ^= s[0];
  s[3] ^= s[1];
  s[1] ^= s[2];
  s[0] ^= s[3];
  s[2] ^= t;
  s[3] = rotl64(s[3], 45);
  return result;
}
void cq_xoshiro256ss_fill(uint64_t state[4], uint64_t* dst, size_t count, uint32_t threads) {
  cq::xoshiro_fill(state, dst, count, threads);
}
uint64_t cq_buffer_rng_next_u64(void* st) {
  cq_buffer_rng* b = (cq_buffer_rng*)st;
  if (b->pos >= b->len) {
    b->overrun++;
    return 0;
  }
  return b->words[b->pos++];
}
// not compared against by the prover: an "unknown" generator as a caller's RngCore is
uint64_t cq_opaque_rng_next_u64(void* st) { return cq_xoshiro256ss_next_u64(st); }
void cq_opaque_rng_fill(void* st, uint64_t* dst, size_t count) { cq::xoshiro_fill((uint64_t*)st, dst, count, 8); }

}  // extern "C"

// ---- permutation::keygen::Assembly (permutation/keygen.rs:14-113), host bookkeeping ---------------------------
void cq_permutation_assembly_init(uint32_t columns, uint32_t n, uint32_t* mapping, uint32_t* aux, uint32_t* sizes) {
  // every cell starts as its own 1-cycle: mapping == aux == identity (:22-41)
  for (uint32_t col = 0; col < columns; col++)
    for (uint32_t r = 0; r < n; r++) {
      const size_t cell = (size_t)col * n + r;
      mapping[2 * cell] = aux[2 * cell] = col;
      mapping[2 * cell + 1] = aux[2 * cell + 1] = r;
      sizes[cell] = 1;
    }
}

int cq_permutation_assembly_copy(uint32_t columns, uint32_t n, uint32_t* mapping, uint32_t* aux, uint32_t* sizes,
                                 uint32_t left_column, uint32_t left_row, uint32_t right_column, uint32_t right_row) {
  if (!mapping || !aux || !sizes) return CQ_ERR_ARG;
  if (left_column >= columns || right_column >= columns) return CQ_ERR_ARG;  // Error::ColumnNotInPermutation
  if (left_row >= n || right_row >= n) return CQ_ERR_ARG;                    // Error::BoundsFailure (:62-66)
  auto cell = [&](uint32_t col, uint32_t row) { return (size_t)col * n + row; };
  size_t left = cell(left_column, left_row), right = cell(right_column, right_row);
  size_t left_cycle = cell(aux[2 * left], aux[2 * left + 1]);
  size_t right_cycle = cell(aux[2 * right], aux[2 * right + 1]);
  if (left_cycle == right_cycle) return CQ_OK;  // already in the same cycle (:75-77)
  if (sizes[left_cycle] < sizes[right_cycle]) std::swap(left_cycle, right_cycle);
  // merge the right cycle into the left one (:83-93)
  sizes[left_cycle] += sizes[right_cycle];
  const uint32_t lc_col = (uint32_t)(left_cycle / n), lc_row = (uint32_t)(left_cycle % n);
  size_t i = right_cycle;
  do {
    aux[2 * i] = lc_col;
    aux[2 * i + 1] = lc_row;
    i = cell(mapping[2 * i], mapping[2 * i + 1]);
  } while (i != right_cycle);
  std::swap(mapping[2 * left], mapping[2 * right]);  // :95-97
  std::swap(mapping[2 * left + 1], mapping[2 * right + 1]);
  return CQ_OK;
}

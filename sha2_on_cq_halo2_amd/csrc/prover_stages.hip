// ---- the same stages for a caller that keeps its own create_proof (capi_rounds.hip checks the arguments) ------------------
// Each runs the shared stage body ProofRun's own stage runs (prover_run.hpp), on caller-owned buffers.
#include "prover_run.hpp"

namespace cq {

using namespace prover;

namespace {

// `count` scalars as Fr::random draws them, through the caller's bulk hook when the key has one
void draw_scalars(Rng& rng, Fr* out, size_t count) {
  std::vector<uint64_t> w(8 * count);
  rng.fill(w.data(), w.size());
  for (size_t i = 0; i < count; i++) out[i] = Fr::from_u512(w.data() + 8 * i);
}

void affine_to_limbs(const G1Affine& p, uint64_t* out) {
  p.x.to_limbs64(out);
  p.y.to_limbs64(out + 4);
}

// commit_lagrange of `count` vectors of n values, one behind the other, as affine points on the host; then each in
// coefficient form in place (waits for the stream: what the caller reads next is there)
int commit_then_coeff(cq_pk* pk, Fr* z, size_t count, uint64_t* commitments) {
  const size_t n = (size_t)1 << pk->k;
  std::vector<const Fr*> sc(count);
  std::vector<const G1Affine*> bs(count, pk->params->g_lagrange);
  for (size_t i = 0; i < count; i++) sc[i] = z + i * n;
  std::vector<G1Affine> o;
  CQ_TRY(commit_batch(pk, sc, bs, n, o));
  for (size_t i = 0; i < count; i++) affine_to_limbs(o[i], commitments + 8 * i);
  CQ_TRY(domain_lagrange_to_coeff(pk->domain, z, z, (uint32_t)count, n, n));
  return pk->ctx->wait(pk->ctx->stream);
}

}  // namespace

int stage_permutation_commit(cq_pk* pk, const uint64_t* const* advice_dev, const uint64_t* const* instance_dev, const Fr& beta,
                             const Fr& gamma, cq_rng_next_u64 rng_next, void* rng_state, Fr* z, uint64_t* commitments) {
  cq_ctx* c = pk->ctx;
  const size_t n = (size_t)1 << pk->k, S = pk->perm_sets(), PC = pk->perm_columns.size();
  const uint32_t bf = pk->bf;
  std::vector<const Fr*> cols(PC);
  for (size_t ci = 0; ci < PC; ci++) {
    const auto& col = pk->perm_columns[ci];
    cols[ci] = col.first == CQ_COL_ADVICE ? (const Fr*)advice_dev[col.second]
             : col.first == CQ_COL_FIXED  ? pk->fixed_values + (size_t)col.second * n
                                          : (const Fr*)instance_dev[col.second];
    if (!cols[ci]) return c->fail(CQ_ERR_ARG, "permutation_commit: a permutation column is NULL");
  }
  void* mv;
  CQ_TRY(c->ensure_scratch(Scratch::ProverStage, S * n * sizeof(Fr), &mv));
  // per set: bf blinding rows, then the blind (permutation/prover.rs:169-175)
  Rng rng{rng_next, rng_state, pk->rng_fill, &c->pool()};
  std::vector<Fr> tails(S * bf), drawn(bf + 1);
  for (size_t st = 0; st < S; st++) {
    draw_scalars(rng, drawn.data(), bf + 1);
    std::copy(drawn.begin(), drawn.begin() + bf, tails.begin() + st * bf);
  }
  CQ_TRY(perm_products(pk, cols.data(), beta, gamma, tails.data(), (Fr*)mv, z));
  return commit_then_coeff(pk, z, S, commitments);  // :177-179
}

int stage_lookup_commit_product(cq_pk* pk, const uint64_t* const* input_dev, const uint64_t* const* table_dev,
                                const uint64_t* const* permuted_input_dev, const uint64_t* const* permuted_table_dev, const Fr& beta,
                                const Fr& gamma, cq_rng_next_u64 rng_next, void* rng_state, Fr* z, uint64_t* commitments) {
  cq_ctx* c = pk->ctx;
  const size_t n = (size_t)1 << pk->k, PL = pk->legacy.size();
  const uint32_t bf = pk->bf;
  Rng rng{rng_next, rng_state, pk->rng_fill, &c->pool()};
  std::vector<Fr> tails(PL * bf), drawn(bf + 1);
  for (size_t l = 0; l < PL; l++) {  // per lookup: bf blinding rows, then the blind
    draw_scalars(rng, drawn.data(), bf + 1);
    std::copy(drawn.begin(), drawn.begin() + bf, tails.begin() + l * bf);
  }
  for (size_t l = 0; l < PL; l++)
    CQ_TRY(lookup_product(c, (const Fr*)input_dev[l], (const Fr*)table_dev[l], (const Fr*)permuted_input_dev[l], (const Fr*)permuted_table_dev[l],
                          beta, gamma, tails.data() + l * bf, (uint32_t)n, bf, z + l * n));
  return commit_then_coeff(pk, z, PL, commitments);
}

int stage_evaluate_h(cq_pk* pk, const uint64_t* const* advice_coeff_dev, const uint64_t* const* instance_coeff_dev, const Fr* perm_z,
                     const uint64_t* const* permuted_input_coeff_dev, const uint64_t* const* permuted_table_coeff_dev, const Fr* lookup_z,
                     const uint64_t* challenges, const Fr& beta, const Fr& gamma, const Fr& theta, const Fr& y, Fr* h_out) {
  cq_ctx* c = pk->ctx;
  cq_domain* dom = pk->domain;
  const hipStream_t s = c->stream;
  const size_t n = (size_t)1 << pk->k, ext = dom->ext(), A = pk->num_advice, I = pk->num_instance, S = pk->perm_sets();
  const size_t PL = pk->legacy.size(), NC = pk->challenge_phase.size();
  if (!pk->general()) {  // nothing to fold: the static lookups are cq_quotient_dev's
    CQ_HIP(c, hipMemsetAsync(h_out, 0, ext * sizeof(Fr), s));
    return CQ_OK;
  }
  void* scr;
  CQ_TRY(c->ensure_scratch(Scratch::ProverStage, ((A + I + S + 5 * PL) * ext + 3 * PL * n + NC + 8) * sizeof(Fr), &scr));
  Fr* adv_cosets = (Fr*)scr;
  Fr* inst_cosets = adv_cosets + A * ext;
  Fr* z_cosets = inst_cosets + I * ext;
  Fr* plk_cosets = z_cosets + S * ext;
  Fr* plk = plk_cosets + 5 * PL * ext;  // per legacy lookup: a', s', z side by side (one batched transform)
  Fr* chal = plk + 3 * PL * n;
  for (size_t a = 0; a < A; a++) CQ_TRY(domain_coeff_to_extended(dom, (const Fr*)advice_coeff_dev[a], adv_cosets + a * ext, 1, n, ext));
  for (size_t i = 0; i < I; i++) CQ_TRY(domain_coeff_to_extended(dom, (const Fr*)instance_coeff_dev[i], inst_cosets + i * ext, 1, n, ext));
  if (S) CQ_TRY(domain_coeff_to_extended(dom, perm_z, z_cosets, (uint32_t)S, n, ext));
  std::vector<const Fr*> plk_polys(PL);
  for (size_t l = 0; l < PL; l++) {
    Fr* p3 = plk + 3 * l * n;
    CQ_HIP(c, hipMemcpyAsync(p3, permuted_input_coeff_dev[l], n * sizeof(Fr), hipMemcpyDeviceToDevice, s));
    CQ_HIP(c, hipMemcpyAsync(p3 + n, permuted_table_coeff_dev[l], n * sizeof(Fr), hipMemcpyDeviceToDevice, s));
    CQ_HIP(c, hipMemcpyAsync(p3 + 2 * n, lookup_z + l * n, n * sizeof(Fr), hipMemcpyDeviceToDevice, s));
    plk_polys[l] = p3;
  }
  if (NC) {
    std::vector<Fr> ch(NC);
    for (size_t i = 0; i < NC; i++) ch[i] = Fr::from_limbs64(challenges + 4 * i);
    CQ_HIP(c, hipMemcpyAsync(chal, ch.data(), NC * sizeof(Fr), hipMemcpyHostToDevice, s));
    CQ_TRY(c->wait(s));  // `ch` is on this frame
  }
  HTermsArgs ht;
  ht.adv_cosets = adv_cosets;
  ht.inst_cosets = inst_cosets;
  ht.z_cosets = z_cosets;
  ht.challenges = chal;
  ht.plk_polys = plk_polys.data();
  ht.plk_cosets = plk_cosets;
  ht.beta = beta;
  ht.gamma = gamma;
  ht.theta = theta;
  ht.y = y;
  return h_terms(pk, ht, h_out);
}

int stage_multiopen(cq_pk* pk, const cq_open_query* queries, size_t count, const cq_open_transcript* transcript) {
  cq_ctx* c = pk->ctx;
  const size_t n = (size_t)1 << pk->k;
  const bool shplonk = pk->opener == CQ_OPENER_SHPLONK;
  // distinct points by value, first-seen order (gwc.rs:36-61, shplonk.rs:56-133)
  std::vector<Query> qs(count);
  std::vector<Fr> points;
  for (size_t i = 0; i < count; i++) {
    const Fr pt = Fr::from_limbs64(queries[i].point);
    size_t g = 0;
    while (g < points.size() && !(points[g] - pt).is_zero()) g++;
    if (g == points.size()) points.push_back(pt);
    qs[i] = {(const Fr*)queries[i].poly_dev, (uint32_t)queries[i].len, 0, -1, Fr::zero(), (uint32_t)g};
  }
  void* scr;
  CQ_TRY(c->ensure_scratch(Scratch::ProverStage, (shplonk ? 5 * n + 64 * 8 : 2 * points.size() * n) * sizeof(Fr), &scr));
  // the evaluations (plonk/prover.rs:654-719 computes them before the opener is called): chunked Horner, per point
  for (size_t g = 0; g < points.size(); g++) {
    std::vector<const Fr*> ps;
    std::vector<uint32_t> ls;
    std::vector<size_t> idx;
    for (size_t i = 0; i < count; i++)
      if (qs[i].pt == g) {
        ps.push_back(qs[i].p);
        ls.push_back(qs[i].len);
        idx.push_back(i);
      }
    std::vector<Fr> ev(ps.size());
    CQ_TRY(eval_many(c, ps, ls, points[g], ev.data()));
    for (size_t m = 0; m < idx.size(); m++) qs[idx[m]].eval = ev[m];
  }
  const std::vector<size_t> no_pieces;
  OpenJob j;
  j.pk = pk;
  j.qs = &qs;
  j.points = &points;
  j.q_h = &no_pieces;
  j.xn = Fr::one();
  j.gwc_batch = (Fr*)scr;
  j.gwc_wit = (Fr*)scr + points.size() * n;
  j.shplonk = (Fr*)scr;
  j.tr.squeeze = [&](Fr& out) {
    uint64_t limbs[4];
    if (transcript->squeeze_challenge(transcript->user, limbs) != 0) return c->fail(CQ_ERR_ARG, "multiopen: the squeeze_challenge callback failed");
    out = Fr::from_limbs64(limbs);
    return (int)CQ_OK;
  };
  j.tr.write_point = [&](const G1Affine& p, const char* what) {
    if (p.is_identity()) return c->fail(CQ_ERR_TRANSCRIPT, what);  // transcript.rs:221-233
    uint64_t limbs[8];
    affine_to_limbs(p, limbs);
    if (transcript->write_point(transcript->user, limbs) != 0) return c->fail(CQ_ERR_ARG, "multiopen: the write_point callback failed");
    return (int)CQ_OK;
  };
  return shplonk ? open_shplonk_queries(j) : open_gwc_queries(j);
}

}  // namespace cq

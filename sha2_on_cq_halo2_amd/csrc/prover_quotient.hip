// The grand products and the quotient: permutation and legacy-lookup products, the non-CQ terms of evaluate_h (the three
// shared stage bodies of prover_run.hpp), and ProofRun's permutation_commit, evaluate_h and construct_h.
#include "prover_run.hpp"

namespace cq {
namespace prover {

// permutation::Argument::commit (permutation/prover.rs:47-198) up to the Lagrange values of every z.  cols[ci]: the
// Lagrange values of permutation column ci; z_tails: sets x bf blinding rows (host, :169-171); mv, z: sets x n each.
int perm_products(const cq_pk* pk, const Fr* const* cols, const Fr& beta, const Fr& gamma, const Fr* z_tails, Fr* mv, Fr* z) {
  cq_ctx* c = pk->ctx;
  const hipStream_t s = c->stream;
  const size_t n = (size_t)1 << pk->k, S = pk->perm_sets(), PC = pk->perm_columns.size(), chunk_len = pk->cs_degree - 2;
  const uint32_t bf = pk->bf, u = pk->u;
  const Fr delta = fr_from_raw(FR_DELTA_RAW);
  std::vector<PermProductArgs> pa(S);
  Fr deltaomega = Fr::one();  // delta^(column position), :86-87,146
  for (size_t st = 0; st < S; st++) {
    PermProductArgs& a = pa[st];
    a.count = (uint32_t)std::min(chunk_len, PC - st * chunk_len);
    a.beta = beta;
    a.gamma = gamma;
    a.omega_powers = pk->omega_powers;
    for (uint32_t j = 0; j < a.count; j++) {
      const size_t ci = st * chunk_len + j;
      a.col[j] = cols[ci];
      a.sigma[j] = pk->perm_values + ci * n;
      a.delta_beta[j] = deltaomega * beta;
      deltaomega = deltaomega * delta;
    }
    CQ_TRY(perm_denominators(c, a, (uint32_t)n, mv + st * n));  // :106-121
  }
  CQ_TRY(poly_batch_invert(c, mv, (uint32_t)(S * n)));  // :124
  for (size_t st = 0; st < S; st++) CQ_TRY(perm_numerators(c, pa[st], (uint32_t)n, mv + st * n));  // :128-147
  // z[0] = last_z, z[row] = z[row-1] * mv[row-1] (:160-166): a multiplicative scan per set, then the
  // chain last_z = z[n - (bf+1)] of the previous set (:173) as one scalar per set
  CQ_TRY(prefix_product(c, mv, z, (uint32_t)n, (uint32_t)S));
  std::vector<Fr> at_u(S);
  for (size_t st = 0; st < S; st++) CQ_HIP(c, hipMemcpyAsync(&at_u[st], z + st * n + u, sizeof(Fr), hipMemcpyDeviceToHost, s));
  CQ_TRY(c->wait(s));
  PermScaleArgs sa;
  Fr last_z = Fr::one();
  for (size_t st = 0; st < S; st++) {
    sa.mult[st] = last_z;
    last_z = last_z * at_u[st];
  }
  CQ_TRY(perm_scale(c, z, (uint32_t)n, u + 1, (uint32_t)S, sa));
  // blinding rows (:169-171)
  for (size_t st = 0; st < S; st++)
    CQ_HIP(c, hipMemcpyAsync(z + st * n + (n - bf), z_tails + st * bf, bf * sizeof(Fr), hipMemcpyHostToDevice, s));
  return CQ_OK;
}

// lookup::Permuted::commit_product (lookup/prover.rs:163-300) up to the Lagrange values of z: the running product of
// (A + beta)(S + gamma) / ((a' + beta)(s' + gamma)), rows n - bf .. from `tails` (host, bf elements).  All vectors: n.
int lookup_product(cq_ctx* c, const Fr* cin, const Fr* ctab, const Fr* perm_in, const Fr* perm_tab, const Fr& beta, const Fr& gamma,
                   const Fr* tails, uint32_t n, uint32_t bf, Fr* z) {
  CQ_TRY(lookup_denominators(c, perm_in, perm_tab, beta, gamma, n, z));
  CQ_TRY(poly_batch_invert(c, z, n));
  CQ_TRY(lookup_numerators(c, cin, ctab, beta, gamma, n, z));
  CQ_TRY(prefix_product(c, z, z, n, 1));
  CQ_HIP(c, hipMemcpyAsync(z + (n - bf), tails, bf * sizeof(Fr), hipMemcpyHostToDevice, c->stream));
  return CQ_OK;
}

// The non-CQ part of Evaluator::evaluate_h (evaluation.rs:285-531): custom gates, permutation terms, legacy-lookup terms,
// folded with y in that order into h_ext.  The columns come on the extended coset already (their transforms are the
// caller's to place); the legacy lookups' a', s', z come as coefficients and are extended here.  A key without any of
// the three (CQ-only) leaves h_ext untouched.
int h_terms(const cq_pk* pk, const HTermsArgs& t, Fr* h_ext) {
  cq_ctx* c = pk->ctx;
  cq_domain* dom = pk->domain;
  const size_t n = (size_t)1 << pk->k, ext = dom->ext(), S = pk->perm_sets(), PC = pk->perm_columns.size();
  const uint32_t rot_scale = 1u << (dom->extended_k - dom->k);
  if (!pk->general()) return CQ_OK;
  GateEvalArgs coset_eval;  // `evaluate` over the extended coset: the gates folded with y, a legacy lookup's expressions with theta
  coset_eval.constants = pk->constants;
  coset_eval.challenges = t.challenges;
  coset_eval.advice = t.adv_cosets;
  coset_eval.fixed = pk->fixed_cosets;
  coset_eval.instance = t.inst_cosets;
  coset_eval.stride = ext;
  coset_eval.size = (uint32_t)ext;
  coset_eval.rot_scale = rot_scale;
  if (pk->num_gate_polys) {  // custom gates (:348-365)
    GateEvalArgs ga = coset_eval;
    ga.prog = pk->gate_prog;
    ga.num_polys = pk->num_gate_polys;
    ga.y = t.y;
    CQ_TRY(gate_eval(c, ga, h_ext));
  } else {
    CQ_HIP(c, hipMemsetAsync(h_ext, 0, ext * sizeof(Fr), c->stream));
  }
  if (S) {  // permutation constraints (:367-459)
    PermHArgs ph;
    ph.z = t.z_cosets;
    ph.sigma = pk->perm_cosets;
    for (size_t ci = 0; ci < PC; ci++) {
      const auto& col = pk->perm_columns[ci];
      ph.col[ci] = col.first == CQ_COL_ADVICE ? t.adv_cosets + (size_t)col.second * ext
                 : col.first == CQ_COL_FIXED  ? pk->fixed_cosets + (size_t)col.second * ext
                                              : t.inst_cosets + (size_t)col.second * ext;
    }
    ph.sets = (uint32_t)S;
    ph.chunk_len = pk->cs_degree - 2;
    ph.ncols = (uint32_t)PC;
    ph.l0 = pk->l0;
    ph.l_last = pk->l_last;
    ph.l_active = pk->l_active_row;
    ph.beta = t.beta;
    ph.gamma = t.gamma;
    ph.y = t.y;
    ph.delta_start = t.beta * dom->g_coset;  // beta * ZETA (:375)
    ph.ext_pow_lo = pk->ext_pow_lo;
    ph.ext_pow_hi = pk->ext_pow_hi;
    ph.delta = fr_from_raw(FR_DELTA_RAW);
    ph.ext = (uint32_t)ext;
    ph.rot_scale = rot_scale;
    ph.last_rot = pk->bf + 1;
    CQ_TRY(perm_h_terms(c, ph, h_ext));
  }
  for (size_t l = 0; l < pk->legacy.size(); l++) {  // legacy lookup constraints (:461-531)
    const auto& lk = pk->legacy[l];
    Fr* co = t.plk_cosets + l * 5 * ext;  // a', s', z cosets, then the compressed input / table on the coset
    CQ_TRY(domain_coeff_to_extended(dom, t.plk_polys[l], co, 3, n, ext));
    for (int side = 0; side < 2; side++) {
      GateEvalArgs ga = coset_eval;
      ga.prog = pk->legacy_prog + (side ? lk.tab_off : lk.in_off);
      ga.num_polys = lk.width;
      ga.y = t.theta;
      CQ_TRY(gate_eval(c, ga, co + (3 + side) * ext));
    }
    LookupHArgs la;
    la.a = co;
    la.s = co + ext;
    la.z = co + 2 * ext;
    la.cin = co + 3 * ext;
    la.ctab = co + 4 * ext;
    la.l0 = pk->l0;
    la.l_last = pk->l_last;
    la.l_active = pk->l_active_row;
    la.beta = t.beta;
    la.gamma = t.gamma;
    la.y = t.y;
    la.ext = (uint32_t)ext;
    la.rot_scale = rot_scale;
    CQ_TRY(lookup_h_terms(c, la, h_ext));
  }
  return CQ_OK;
}

// ---- permutation::Argument::commit (permutation/prover.rs:47-198): Lagrange values of every z ----------
int ProofRun::permutation_commit() {
  if (!S) return CQ_OK;
  std::vector<const Fr*> cols(PC);
  for (size_t ci = 0; ci < PC; ci++) {
    const auto& col = pk->perm_columns[ci];
    cols[ci] = col.first == CQ_COL_ADVICE ? B.adv + (size_t)col.second * n
             : col.first == CQ_COL_FIXED  ? pk->fixed_values + (size_t)col.second * n
                                          : B.inst_lag + (size_t)col.second * n;
  }
  return perm_products(pk, cols.data(), beta, gamma, z_tails.data(), B.mv, B.z);
}

// ---- evaluate_h (evaluation.rs:285-551) + divide by the vanishing polynomial ------------------------
int ProofRun::evaluate_h() {
  if (general) {
    // advice / instance cosets (:317-335), permutation product cosets (permutation/prover.rs:182)
    if (I && !(L || PL)) CQ_TRY(coeff_to_extended_cols(B.inst_coeff, B.inst_cosets, I));  // no round 1
    if (S) CQ_TRY(coeff_to_extended_cols(B.z, B.z_cosets, S));
    std::vector<const Fr*> plk_polys(PL);
    for (size_t l = 0; l < PL; l++) plk_polys[l] = plk_buf(l, 2);
    HTermsArgs ht;
    ht.adv_cosets = B.adv_cosets;
    ht.inst_cosets = B.inst_cosets;
    ht.z_cosets = B.z_cosets;
    ht.challenges = B.challenges;
    ht.plk_polys = plk_polys.data();
    ht.plk_cosets = B.plk_cosets;
    ht.beta = beta;
    ht.gamma = gamma;
    ht.theta = theta;
    ht.y = y;
    CQ_TRY(h_terms(pk, ht, B.h_ext));  // gates, permutation, legacy lookups (:348-531)
  }
  // CQ terms (:533-548), then the division by X^n - 1 (vanishing/prover.rs:84, domain.rs:319-338)
  CqQuotientArgs qa;
  qa.h_in = general ? B.h_ext : nullptr;
  qa.l_active = pk->l_active_row;
  qa.t_evals = dom->t_evaluations_dev;
  qa.t_len = (uint32_t)dom->t_evaluations.size();
  qa.y = y;
  qa.beta = beta;
  if (resident) return resident_quotient(qa);
  qa.count = (uint32_t)L;
  for (size_t l = 0; l < L; l++) {
    qa.b[l] = B.cosets + l * ext;
    qa.f[l] = B.cosets + (L + l) * ext;
  }
  return poly_cq_quotient(c, qa, (uint32_t)ext, B.h_ext);
}

// vanishing.construct (vanishing/prover.rs:69-120): coefficients, n-sized pieces, blinds, commitments
int ProofRun::construct_h() {
  if (resident) CQ_TRY(resident_collect_h());
  else CQ_TRY(domain_extended_to_coeff(dom, B.h_ext, B.h_coeff));
  for (size_t i = 0; i < pieces; i++) (void)rng.fr();  // h_blinds (:95-98)
  {
    std::vector<const Fr*> sc(pieces);
    std::vector<const G1Affine*> bs(pieces, pk->params->g);
    for (size_t i = 0; i < pieces; i++) sc[i] = B.h_coeff + i * n;
    std::vector<G1Affine> o;
    CQ_TRY(commit_batch(pk, sc, bs, n, o));
    for (auto& p : o)
      if (!tr.write_point(p)) return c->fail(CQ_ERR_TRANSCRIPT, "h piece commitment is the identity");
  }
  return CQ_OK;
}

}  // namespace prover
}  // namespace cq

// Resident column sharding (cq_pk_set_resident_sharding; DESIGN.md, multi-GPU), all of it: where a proof over a sharded
// key departs from the replicated flow, the stage (named in each comment) hands over to one of these methods.  A
// transformed column stays on its owner and only slices travel: ownership is by contiguous ranges (shard_range) of the
// lookups (lk_lo, lk_hi) and of the advice columns (adv_lo, adv_hi); consumers go by point range (my_lo, my_hi), as the
// MSMs are cut.  Received slices land in the staging buffer set-up reserves (res_stage_v).  Every rank derives the same
// transcript.
#include "prover_run.hpp"

namespace cq {
namespace prover {

uint32_t ProofRun::owner_of(size_t item, size_t count) const {
  for (uint32_t r = 0; r < SW; r++) {
    size_t lo, hi;
    shard_range(count, r, SW, lo, hi);
    if (item >= lo && item < hi) return r;
  }
  return 0;
}

// the constructor: which circuits qualify, and this rank's ranges of the lookups and the advice columns
void ProofRun::resident_init() {
  resident = shard_resident_enabled(pk) && !general && PL == 0 && pk->num_phases == 1 && pk->challenge_phase.empty() && I == 0 &&
             L > 0 && pk->opener == CQ_OPENER_GWC && n >= (size_t)64 * pk->shard_world;
  for (size_t l = 0; l < L && resident; l++)
    for (int64_t pj : pk->lookups[l].prog) resident = resident && pj < 0;
  if (resident) {
    shard_range(L, me, SW, lk_lo, lk_hi);
    shard_range(A, me, SW, adv_lo, adv_hi);
  }
  lk_cnt = lk_hi - lk_lo;
}

// setup: where received slices land (res_stage_elems: see the member's comment)
int ProofRun::resident_reserve_staging() { return c->ensure_scratch(Scratch::ProverStage, res_stage_elems * sizeof(Fr), &res_stage_v); }

// advice_phase, on the side stream: the owner transforms its advice columns
int ProofRun::resident_advice_to_coeff() {
  if (adv_hi > adv_lo) CQ_TRY(domain_lagrange_to_coeff(dom, B.adv + adv_lo * n, adv_poly + adv_lo * n, (uint32_t)(adv_hi - adv_lo), n, n));
  return CQ_OK;
}

// cq_round1, on the side stream
int ProofRun::resident_round1_transforms() {
  // resident: the owner transforms its lookups' f and its advice columns; nobody else ever reads them
  if (lk_cnt) {
    CQ_TRY(domain_lagrange_to_coeff(dom, B.f_lag + lk_lo * n, B.f_coeff + lk_lo * n, (uint32_t)lk_cnt, n, n));
    CQ_TRY(domain_coeff_to_extended(dom, B.f_coeff + lk_lo * n, B.cosets + (L + lk_lo) * ext, (uint32_t)lk_cnt, n, ext));
  }
  if (!adv_is_coeff && adv_hi > adv_lo) CQ_TRY(domain_lagrange_to_coeff(dom, B.adv + adv_lo * n, B.adv + adv_lo * n, (uint32_t)(adv_hi - adv_lo), n, n));
  adv_is_coeff = true;
  return CQ_OK;
}

// round2_prepare: the inversions, b on the owner only
int ProofRun::resident_round2_invert() {
  if (lk_cnt) CQ_TRY(poly_batch_invert(c, B.bpoly + lk_lo * n, (uint32_t)(lk_cnt * n)));
  CQ_TRY(poly_batch_invert(c, B.den, (uint32_t)(L * N)));  // the table side is small and stays replicated
  return CQ_OK;
}

// round2_prepare: b -> coefficients, b(0) on its way to the host, the slices of b_0 to their consumers
int ProofRun::resident_round2_b_to_coeff() {
  // resident: the owner turns its b_l into coefficients; every rank commits its point range of b_0 = (b - b(0)) / X
  // (:279, 299, 310: the same coefficients over two base arrays), so slice r of b_l[1..n) goes from the owner to rank r
  if (lk_cnt) CQ_TRY(domain_lagrange_to_coeff(dom, B.bpoly + lk_lo * n, B.bpoly + lk_lo * n, (uint32_t)lk_cnt, n, n));
  for (size_t l = 0; l < L; l++) small_fr[l] = Fr::zero();
  if (lk_cnt) {
    GatherArgs ga;
    ga.count = (uint32_t)lk_cnt;
    for (size_t l = lk_lo; l < lk_hi; l++) ga.src[l - lk_lo] = B.bpoly + l * n;
    CQ_TRY(poly_gather_scalars(c, ga, B.gather));
    CQ_HIP(c, hipMemcpyAsync(small_fr + lk_lo, B.gather, lk_cnt * sizeof(Fr), hipMemcpyDeviceToHost, s));  // summed over the ranks below
  }
  std::vector<Xfer> xf;
  for (size_t l = 0; l < L; l++) {
    const uint32_t own = owner_of(l, L);
    for (uint32_t r = 0; r < SW; r++) {
      size_t lo, hi;
      shard_range(n - 1, r, SW, lo, hi);
      Fr* p = B.bpoly + l * n + 1 + lo;
      if (hi > lo) xf.push_back({p, p, (hi - lo) * sizeof(Fr), own, r});
    }
  }
  CQ_TRY(shard_exchange(pk, xf.data(), xf.size(), s));
  return CQ_OK;
}

// round2_commit, on the side stream: b_l's coset stays with the owner of lookup l (the quotient is folded there)
int ProofRun::resident_b_to_coset() {
  if (lk_cnt) CQ_TRY(domain_coeff_to_extended(dom, B.bpoly + lk_lo * n, B.cosets + lk_lo * ext, (uint32_t)lk_cnt, n, ext));
  return CQ_OK;
}

// round2_commit: every b_l(0) from its owner
int ProofRun::resident_sum_b_at_zero() { return shard_sum_scalars(pk, small_fr, L); }

// evaluate_h: the CQ terms of the owned lookups (`qa` comes with everything but the lookups filled in)
int ProofRun::resident_quotient(CqQuotientArgs& qa) {
  qa.count = (uint32_t)lk_cnt;
  for (size_t l = 0; l < qa.count; l++) {
    qa.b[l] = B.cosets + (lk_lo + l) * ext;
    qa.f[l] = B.cosets + (L + lk_lo + l) * ext;
  }
  // resident: the numerator is a sum over lookups (evaluation.rs:533-548 folds them with powers of y), each owner
  // folds its own range and multiplies by the power of y the lookups after its range contribute
  qa.scale = y.pow_u64(L - lk_hi);
  qa.has_scale = 1;
  if (lk_cnt) CQ_TRY(poly_cq_quotient(c, qa, (uint32_t)ext, B.h_ext));
  return CQ_OK;
}

// construct_h: h's coefficients, on this rank's point range
int ProofRun::resident_collect_h() {
  if (lk_cnt) CQ_TRY(domain_extended_to_coeff(dom, B.h_ext, B.h_coeff));
  // resident: division by X^n - 1, extended_to_coeff and the commitments are all linear, so each owner transformed its
  // PARTIAL quotient; rank r now collects slice r of every piece from every owner and adds them up -- it holds the
  // coefficients of h on its own point range only (which is all its share of the commitments, evaluations and the
  // opening reads).  Staging: the buffer reserved at set-up.
  const size_t slice_max = res_slice_max;
  Fr* const stage = (Fr*)res_stage_v;
  std::vector<uint32_t> owners;  // ranks that own a lookup
  for (uint32_t q = 0; q < SW; q++) {
    size_t lo, hi;
    shard_range(L, q, SW, lo, hi);
    if (hi > lo) owners.push_back(q);
  }
  if (owners.size() * pieces * slice_max > res_stage_elems) return c->fail(CQ_ERR_INTERNAL, "resident sharding: staging too small");
  std::vector<Xfer> xf;
  for (size_t oi = 0; oi < owners.size(); oi++)
    for (size_t i = 0; i < pieces; i++)
      for (uint32_t r = 0; r < SW; r++) {
        size_t lo, hi;
        shard_range(n, r, SW, lo, hi);
        if (hi > lo) xf.push_back({B.h_coeff + i * n + lo, stage + (oi * pieces + i) * slice_max, (hi - lo) * sizeof(Fr), owners[oi], r});
      }
  CQ_TRY(shard_exchange(pk, xf.data(), xf.size(), s));
  size_t lo, hi;
  shard_range(n, me, SW, lo, hi);
  for (size_t i = 0; i < pieces && hi > lo; i++) {
    std::vector<Term> terms;
    for (size_t oi = 0; oi < owners.size(); oi++) terms.push_back({stage + (oi * pieces + i) * slice_max, (uint32_t)(hi - lo), Fr::one()});
    CQ_TRY(lincomb_many(c, terms, Fr::zero(), (uint32_t)(hi - lo), B.h_coeff + i * n + lo));
  }
  return CQ_OK;
}

// evaluate_and_write: the evaluation of every query (q_advice, q_b0, q_f: the queries of the advice columns, of each lookup's
// b_0 and of its f).  Who holds what -- an advice polynomial on the owner of its column, b_0 / f of a lookup on its owner (whole
// polynomials, evaluated there), the h pieces and the random polynomial on every rank by point range (each rank
// evaluates its range and multiplies by x^lo).  qowner[i] = owning rank, or -1 for "by point range".
int ProofRun::resident_evaluate(const std::vector<size_t>& q_advice, const std::vector<size_t>& q_b0, const std::vector<size_t>& q_f) {
  qowner.assign(qs.size(), -1);
  shard_range(n, me, SW, my_lo, my_hi);
  for (size_t j = 0; j < q_advice.size(); j++) qowner[q_advice[j]] = (int)owner_of(pk->advice_queries[j].first, A);
  for (size_t l = 0; l < L; l++) qowner[q_b0[l]] = qowner[q_f[l]] = (int)owner_of(l, L);
  std::vector<const Fr*> ps;
  std::vector<uint32_t> ls;
  std::vector<size_t> idx;
  for (size_t i = 0; i < qs.size(); i++) {
    if (qowner[i] >= 0 && qowner[i] != (int)me) continue;
    const bool whole = qowner[i] >= 0;
    if (!whole && my_hi <= my_lo) continue;
    ps.push_back(whole ? qs[i].p : qs[i].p + my_lo);
    ls.push_back(whole ? qs[i].len : (uint32_t)(my_hi - my_lo));
    idx.push_back(i);
  }
  std::vector<Fr> ev(ps.size()), contrib(qs.size(), Fr::zero());
  if (!ps.empty()) CQ_TRY(eval_many(c, ps, ls, x, ev.data()));
  const Fr x_lo = x.pow_u64(my_lo);
  for (size_t j = 0; j < idx.size(); j++) contrib[idx[j]] = qowner[idx[j]] >= 0 ? ev[j] : ev[j] * x_lo;
  CQ_TRY(shard_sum_scalars(pk, contrib.data(), contrib.size()));  // one all-gather: every evaluation is a sum over the ranks
  for (size_t i = 0; i < qs.size(); i++) qs[i].eval = contrib[i];
  return CQ_OK;
}

// resident: poly_batch = sum_j v^j p_j is assembled where the p_j live -- whole polynomials on their owner, the
// by-range ones on each rank's range -- as a partial sum P_r over all n coefficients; rank r then collects the
// slice of every P_q that its share of the witness polynomial needs and adds them up.  kate_division
// (q_i = a_(i+1) + z q_(i+1)) runs per range: the carry into a range from above is the Horner value of the
// slices above it, S_q = sum_t slice_q[t] z^t, exchanged as one field element per rank.
int ProofRun::resident_witness(size_t g, const std::vector<Term>& terms, const Fr& eval_batch, Fr* batch, Fr* wit) {
  const Fr z = points[g];
  std::vector<Term> whole, ranged;
  size_t ti = 0;
  for (size_t i = 0; i < qs.size(); i++) {
    if (qs[i].pt != g) continue;
    const Term& t = terms[ti++];
    if (qowner[i] < 0) ranged.push_back({t.p + my_lo, (uint32_t)(my_hi - my_lo), t.coeff});
    else if (qowner[i] == (int)me) whole.push_back(t);
  }
  if (whole.empty()) CQ_HIP(c, hipMemsetAsync(batch, 0, n * sizeof(Fr), s));
  else CQ_TRY(lincomb_many(c, whole, Fr::zero(), (uint32_t)n, batch));
  if (my_hi > my_lo) {  // the by-range terms on this rank's range; "- eval_batch" touches coefficient 0 only
    std::vector<Term> tt{{batch + my_lo, (uint32_t)(my_hi - my_lo), Fr::one()}};
    tt.insert(tt.end(), ranged.begin(), ranged.end());
    CQ_TRY(lincomb_many(c, tt, my_lo == 0 ? eval_batch : Fr::zero(), (uint32_t)(my_hi - my_lo), batch + my_lo));
  }
  // rank r commits witness coefficients [wlo, whi) (its point range of the n - 1 term MSM) and needs a[wlo+1 .. whi]
  const size_t slice_max = res_slice_max;
  Fr* const stage = (Fr*)res_stage_v;
  std::vector<Xfer> xf;
  for (uint32_t q = 0; q < SW; q++)
    for (uint32_t r = 0; r < SW; r++) {
      size_t wlo, whi;
      shard_range(n - 1, r, SW, wlo, whi);
      if (whi > wlo) xf.push_back({batch + 1 + wlo, stage + (size_t)q * slice_max, (whi - wlo) * sizeof(Fr), q, r});
    }
  CQ_TRY(shard_exchange(pk, xf.data(), xf.size(), s));
  size_t wlo, whi;
  shard_range(n - 1, me, SW, wlo, whi);
  const size_t len = whi - wlo;
  // [0] unused, [1 .. len] the summed slice, [len + 1] the carry -- behind the received slices in the staging area
  Fr* a_loc = stage + (size_t)SW * slice_max + 8;
  if ((size_t)SW * slice_max + 8 + len + 2 > res_stage_elems) return c->fail(CQ_ERR_INTERNAL, "resident sharding: staging too small");
  Fr slice_eval = Fr::zero();
  if (len) {
    std::vector<Term> tt;
    for (uint32_t q = 0; q < SW; q++) tt.push_back({stage + (size_t)q * slice_max, (uint32_t)len, Fr::one()});
    CQ_TRY(lincomb_many(c, tt, Fr::zero(), (uint32_t)len, a_loc + 1));
    const Fr* pp = a_loc + 1;
    const uint32_t ll = (uint32_t)len;
    CQ_TRY(poly_eval_batch(c, &pp, &ll, 1, z, &slice_eval));
  }
  std::vector<Fr> all_s(SW);
  CQ_TRY(shard_allgather_host(pk, &slice_eval, all_s.data(), sizeof(Fr)));
  Fr carry = Fr::zero();  // q_(whi) = S_(r+1) + z^len_(r+1) (S_(r+2) + ...)
  for (uint32_t q = SW; q-- > me + 1;) {
    size_t qlo, qhi;
    shard_range(n - 1, q, SW, qlo, qhi);
    carry = all_s[q] + z.pow_u64(qhi - qlo) * carry;
  }
  if (len) {
    Fr edge[2] = {Fr::zero(), carry};
    CQ_HIP(c, hipMemcpyAsync(a_loc, &edge[0], sizeof(Fr), hipMemcpyHostToDevice, s));
    CQ_HIP(c, hipMemcpyAsync(a_loc + len + 1, &edge[1], sizeof(Fr), hipMemcpyHostToDevice, s));
    CQ_TRY(c->wait(s));  // `edge` is on this frame
    CQ_TRY(poly_kate_division(c, a_loc, (uint32_t)(len + 2), z, wit + wlo));  // wit[wlo .. whi) (and the carry at [whi])
  }
  return CQ_OK;
}

}  // namespace prover
}  // namespace cq

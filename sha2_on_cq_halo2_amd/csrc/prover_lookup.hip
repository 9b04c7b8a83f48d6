// ProofRun's lookup stages: CQ round 1 (multiplicities, f) and round 2 (a, q_a, a_0, b_0, p, with the vanishing argument's
// random polynomial riding along), and the legacy lookups' permuted columns and grand products.
#include "prover_run.hpp"

namespace cq {
namespace prover {

// `evaluate(expr, n, 1, fixed, advice, instance)`: gate_eval's arguments for `num_polys` expressions over the Lagrange
// basis, folded with `fold` (static_lookup/prover.rs:91-107, lookup/prover.rs:98-117)
GateEvalArgs ProofRun::lagrange_eval_args(const uint32_t* prog, uint32_t num_polys, const Fr& fold) const {
  GateEvalArgs ga;
  ga.prog = prog;
  ga.num_polys = num_polys;
  ga.constants = pk->constants;
  ga.challenges = B.challenges;
  ga.advice = B.adv;
  ga.fixed = pk->fixed_values;
  ga.instance = B.inst_lag;
  ga.stride = n;
  ga.size = (uint32_t)n;
  ga.rot_scale = 1;
  ga.y = fold;
  return ga;
}
// `evaluate(expr, n, 1, ..)` of every expression, folded with theta (lookup/prover.rs:98-117)
int ProofRun::lagrange_compress(const uint32_t* prog, uint32_t width, const Fr& chal, Fr* dst) {
  return gate_eval(c, lagrange_eval_args(prog, width, chal), dst);
}

// ---- CQ round 1, the part that does not depend on theta (static_lookup/prover.rs:91-107, 122-160): the lookup
//      inputs on the Lagrange basis and the multiplicities m.  With a single phase and no user challenge the witness
//      alone determines them, so they are computed right after the advice columns are in place and [m] is committed
//      in the advice launch -- the round then has no launch of its own (unless it has legacy lookups or an f that is
//      not a linear combination of advice columns).  The points are WRITTEN where the reference writes them.
int ProofRun::count_multiplicities() {
  if (!L) return CQ_OK;
  CQ_HIP(c, hipMemsetAsync(B.m_counts, 0, (L * N + 16) * sizeof(uint32_t), s));
  size_t input_slot = 0;
  CqRound1Batch r1b;
  r1b.count = 0;
  for (size_t l = 0; l < L; l++) {
    const cq_lookup_desc& lk = pk->lookups[l];
    const uint32_t w = (uint32_t)lk.cols.size();
    // input expressions on the Lagrange basis: `evaluate(expr, n, 1, fixed, advice, instance)` (:91-107)
    for (uint32_t j = 0; j < w; j++, input_slot++) {
      if (lk.prog[j] < 0) {
        lk_input[l][j] = B.adv + (size_t)lk.cols[j] * n;
        continue;
      }
      Fr* dst = B.lk_inputs + input_slot * n;
      CQ_TRY(gate_eval(c, lagrange_eval_args(pk->lookup_prog + lk.prog[j], 1, Fr::zero()), dst));
      lk_input[l][j] = dst;
    }
    CqRound1Args& ra = r1b.a[r1b.count];
    ra.width = w;
    for (uint32_t j = 0; j < w; j++) {
      ra.cols[j] = lk_input[l][j];
      ra.values[j] = lk.tables[j]->values;
      ra.slots[j] = lk.tables[j]->slots;
      ra.nslots[j] = lk.tables[j]->nslots;
    }
    r1b.bucket[r1b.count] = b_by_rows ? B.b_index + l * n : nullptr;
    r1b.n = b_by_rows ? (uint32_t)n : 0;
    r1b.blind_bucket = (uint32_t)N;
    r1b.m_counts[r1b.count++] = B.m_counts + l * N;
    if (r1b.count == CQ_ROUND1_BATCH || l + 1 == L) {  // the lookups of a proof share launches
      CQ_TRY(cq::cq_round1(c, r1b, u, B.err_dev));
      r1b.count = 0;
    }
  }
  CQ_TRY(cq_m_to_fr(c, B.m_counts, (uint32_t)(L * N), B.m_fr));  // the L vectors are adjacent
  if (!sums_side) CQ_TRY(bucket_sum_launches());  // (otherwise beside the launch that commits [m]: fork_bucket_sums)
  *herr = 0;
  CQ_HIP(c, hipMemcpyAsync((void*)herr, B.err_dev, 4, hipMemcpyDeviceToHost, s));  // read after the next synchronisation
  return CQ_OK;
}
// the per-table-row sums of the key's row bases over cq_round1's bucket indices (b_by_rows), on c->stream
int ProofRun::bucket_sum_launches() {
  for (size_t l0 = 0; b_by_rows && l0 < L; l0 += MSM_MAX_BATCH / 2) {
    std::vector<const uint32_t*> sc;
    std::vector<const G1Affine*> bs;
    for (size_t l = l0; l < std::min(L, l0 + MSM_MAX_BATCH / 2); l++)
      for (int q = 0; q < 2; q++) { sc.push_back(B.b_index + l * n); bs.push_back(pk->b_row_bases[q]); }
    if (msm_bucket_sums(c, sc.data(), bs.data(), (uint32_t)n, (uint32_t)sc.size(), (uint32_t)(N + 1), B.b_sums + 2 * l0 * (N + 1)) != 0)
      return c->fail(CQ_ERR_HIP, "bucket-sum launch failed");
  }
  return CQ_OK;
}
int ProofRun::lookup_error() {
  if (*herr == 1) return c->fail(CQ_ERR_LOOKUP, "witness value not in table");
  if (*herr == 2) return c->fail(CQ_ERR_LOOKUP, "Vector lookup must be on the same table row");
  return CQ_OK;
}

// ---- legacy lookups: commit_permuted (lookup/prover.rs:57-160) ---------------------------------------------
int ProofRun::legacy_commit_permuted() {
  if (!PL) return CQ_OK;
  // permute_expression_pair (lookup/prover.rs:400-502) on the device: canonical values, sorted and matched there
  // (lksort.hip), back to Montgomery form; one status read-back per lookup
  void* stage_v;
  const size_t slot = n * 4;  // u64 words of one array of 2^k canonical values
  CQ_TRY(c->ensure_scratch(Scratch::ProverStage, 3 * slot * sizeof(uint64_t) + lookup_permute_scratch_bytes(k) + 64, &stage_v));
  uint64_t* stage = (uint64_t*)stage_v;
  void* lk_scratch = stage + 3 * slot;
  uint32_t* lk_status = (uint32_t*)((char*)lk_scratch + lookup_permute_scratch_bytes(k));
  uint32_t* lk_status_host = (uint32_t*)((char*)small_v + 16);  // beside the lookup error flag
  for (size_t l = 0; l < PL; l++) {
    const auto& lk = pk->legacy[l];
    CQ_TRY(lagrange_compress(pk->legacy_prog + lk.in_off, lk.width, theta, plk_buf(l, 0)));
    CQ_TRY(lagrange_compress(pk->legacy_prog + lk.tab_off, lk.width, theta, plk_buf(l, 1)));
    CQ_TRY(fr_to_canonical(c, plk_buf(l, 0), u, stage));
    CQ_TRY(fr_to_canonical(c, plk_buf(l, 1), u, stage + slot));
    CQ_TRY(lookup_permute_dev(c, stage, stage + slot, u, k, stage + 2 * slot, lk_scratch, lk_status));
    CQ_HIP(c, hipMemcpyAsync(lk_status_host, lk_status, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    CQ_TRY(fr_from_canonical(c, stage, u, plk_buf(l, 2)));
    CQ_TRY(fr_from_canonical(c, stage + 2 * slot, u, plk_buf(l, 3)));
    CQ_HIP(c, hipMemcpyAsync(plk_buf(l, 2) + u, plk_tails.data() + l * 2 * (bf + 1), (bf + 1) * sizeof(Fr), hipMemcpyHostToDevice, s));
    CQ_HIP(c, hipMemcpyAsync(plk_buf(l, 3) + u, plk_tails.data() + l * 2 * (bf + 1) + (bf + 1), (bf + 1) * sizeof(Fr), hipMemcpyHostToDevice, s));
    CQ_TRY(c->wait(s));  // the staging arrays are reused by the next lookup
    if (lk_status_host[0] != 0 || lk_status_host[1] != lk_status_host[2])
      return c->fail(CQ_ERR_LOOKUP, "lookup input not in table (Error::ConstraintSystemFailure)");
  }
  return CQ_OK;
}

// ---- CQ round 1 (static_lookup/prover.rs:51-183) ------------------------------------------------
int ProofRun::cq_round1() {
  if (L && !early_m) {
    CQ_TRY(count_multiplicities());
    CQ_TRY(c->wait(s));
    CQ_TRY(lookup_error());
  }
  theta_pow[0] = Fr::one();
  for (uint32_t j = 1; j < CQ_MAX_WIDTH; j++) theta_pow[j] = theta_pow[j - 1] * theta;
  for (size_t l0 = 0; l0 < L; l0 += CQ_FOLD_BATCH) {
    // f = sum_j theta^(w-1-j) * e_j   (:108-116, Horner with the first expression first), the lookups of a proof per launch
    CqFoldBatch fb;
    fb.count = (uint32_t)std::min<size_t>(CQ_FOLD_BATCH, L - l0);
    for (uint32_t j = 0; j < CQ_MAX_WIDTH; j++) fb.theta_pow[j] = theta_pow[j];
    for (uint32_t q = 0; q < fb.count; q++) {
      const size_t l = l0 + q;
      const uint32_t w = (uint32_t)pk->lookups[l].cols.size();
      fb.width[q] = w;
      for (uint32_t j = 0; j < w; j++) fb.src[q][j] = lk_input[l][j];
      fb.out[q] = owns_lookup(l) ? B.f_lag + l * n : nullptr;
    }
    CQ_TRY(cq_fold_inputs(c, fb, (uint32_t)n));
  }
  if (L || PL) {
    // permuted input / table of every legacy lookup (lookup/prover.rs:136-151), then f_cm (:165) and, unless it went
    // out with the advice launch, m_cm (:167-172): one launch
    std::vector<const Fr*> sc;
    std::vector<const G1Affine*> bs;
    std::vector<size_t> ln;
    for (size_t l = 0; l < PL; l++)
      for (int which = 2; which <= 3; which++) { sc.push_back(plk_buf(l, which)); bs.push_back(pk->params->g_lagrange); ln.push_back(n); }
    // f_cm: when every input of a lookup is a plain advice column, f = sum_j theta^(w-1-j) e_j over whole columns
    // (blinding rows included), so [f] = sum_j theta^(w-1-j) [e_j] -- w - 1 scalar multiplications of commitments
    // round 0 already produced, done by host threads, instead of an n-term MSM.
    std::vector<int> f_linear(L, 0);
    std::vector<G1Jac> f_host(L);
    for (size_t l = 0; l < L; l++) {
      f_linear[l] = 1;
      for (int64_t pj : pk->lookups[l].prog) f_linear[l] &= pj < 0;
    }
    std::vector<size_t> f_slot(L, 0);
    for (size_t l = 0; l < L; l++)
      if (!f_linear[l]) { f_slot[l] = sc.size(); sc.push_back(B.f_lag + l * n); bs.push_back(pk->params->g_lagrange); ln.push_back(n); }
    const size_t m_first = sc.size();
    if (!early_m)
      for (size_t l = 0; l < L; l++) { sc.push_back(B.m_fr + l * N); bs.push_back(pk->table_cfg->g1_lagrange); ln.push_back(N); }
    std::vector<G1Affine> cm;
    Commit r1;
    const uint64_t seq = c->msm_tail_seq;
    if (!sc.empty()) CQ_TRY(r1.begin(pk, sc, bs, ln));
    if (L && !early_m) CQ_TRY(fork_bucket_sums(seq));
    // (on the context's worker threads: the main thread goes on queueing the work that needs theta only)
    std::vector<size_t> f_lin;
    for (size_t l = 0; l < L; l++)
      if (f_linear[l]) f_lin.push_back(l);
    struct PoolJoin {  // an error path must not leave workers with references into this frame
      HostPool& pool;
      HostPool::Ticket t;
      ~PoolJoin() { pool.wait(t); }
    } f_job{c->pool(), nullptr};
    f_job.t = c->pool().submit(f_lin.size(), [&](size_t i) {
      const size_t l = f_lin[i];
      const auto& lcols = pk->lookups[l].cols;
      G1Jac acc = jac_from_affine(advice_commitments[lcols[0]]);
      for (size_t j = 1; j < lcols.size(); j++) acc = jac_add(host_scalar_mul(acc, theta), jac_from_affine(advice_commitments[lcols[j]]));
      f_host[l] = acc;
    });
    {
      // on the side stream (under the launch's tail when there is one): f -> coefficients (:326-334) and onto the
      // extended coset (evaluation.rs:533-548 reads it), the instance cosets -- none of them depends on beta / gamma
      AuxFork fork(c);
      CQ_TRY(fork.begin(seq));
      if (resident) {
        CQ_TRY(resident_round1_transforms());
      } else {
        if (L) {
          CQ_TRY(lagrange_to_coeff_cols(B.f_lag, B.f_coeff, L));
          CQ_TRY(coeff_to_extended_cols(B.f_coeff, B.cosets + L * ext, L));
        }
        if (general && I) CQ_TRY(coeff_to_extended_cols(B.inst_coeff, B.inst_cosets, I));
        if (A && S == 0 && !adv_is_coeff) {
          // advice -> coefficients (prover.rs:587-603), in place: without a permutation argument nothing reads the
          // Lagrange values after round 1, and the round-2 inversions leave room for it
          CQ_TRY(lagrange_to_coeff_cols(B.adv, B.adv, A));
          adv_is_coeff = true;
        }
      }
      CQ_TRY(fork.end());
    }
    if (!sc.empty()) CQ_TRY(r1.end(cm));
    c->pool().wait(f_job.t);
    for (size_t q = 0; q < 2 * PL; q++)
      if (!tr.write_point(cm[q])) return c->fail(CQ_ERR_TRANSCRIPT, "permuted lookup commitment is the identity");
    for (size_t l = 0; l < L; l++) {
      const G1Affine f_cm = f_linear[l] ? jac_to_affine(f_host[l]) : cm[f_slot[l]];
      if (!tr.write_point(f_cm)) return c->fail(CQ_ERR_TRANSCRIPT, "f commitment is the identity");
      if (!tr.write_point(early_m ? m_commitments[l] : cm[m_first + l])) return c->fail(CQ_ERR_TRANSCRIPT, "m commitment is the identity");
    }
  }
  return CQ_OK;
}

// ---- legacy lookups: commit_product (lookup/prover.rs:163-300): z = running product of
//      (A + beta)(S + gamma) / ((a' + beta)(s' + gamma)), rows n-bf.. random ---------------------------------------
int ProofRun::legacy_commit_product() {
  for (size_t l = 0; l < PL; l++)
    CQ_TRY(lookup_product(c, plk_buf(l, 0), plk_buf(l, 1), plk_buf(l, 2), plk_buf(l, 3), beta, gamma, plkz_tails.data() + l * bf, (uint32_t)n, bf,
                          plk_buf(l, 4)));
  return CQ_OK;
}

// ---- CQ round 2 (static_lookup/prover.rs:187-342) -------------------------------------------------
int ProofRun::cq_round2() {
  bool random_late = false;
  CQ_TRY(round2_prepare());
  CQ_TRY(round2_random_late(random_late));
  return round2_commit(random_late);
}
// round 2, before the launch: denominators, inversions, the values of a, b -> coefficients and b(0) on its way to the host
int ProofRun::round2_prepare() {
  for (size_t l0 = 0; l0 < L; l0 += CQ_FOLD_BATCH) {
    // per lookup: t_i = sum_j theta^(w-1-j) T_j[i] (compress_tables :224-240), den_i = m_i ? t_i + beta : 0 (:245-247),
    // B_r = f_r + beta for r < u, beta on the blinding rows (:261-269) -- one launch for the lookups of the proof
    CqFoldBatch fb;
    fb.count = (uint32_t)std::min<size_t>(CQ_FOLD_BATCH, L - l0);
    for (uint32_t j = 0; j < CQ_MAX_WIDTH; j++) fb.theta_pow[j] = theta_pow[j];
    for (uint32_t q = 0; q < fb.count; q++) {
      const size_t l = l0 + q;
      const cq_lookup_desc& lk = pk->lookups[l];
      fb.width[q] = (uint32_t)lk.cols.size();
      for (uint32_t j = 0; j < fb.width[q]; j++) fb.src[q][j] = lk.tables[j]->values;
      fb.out[q] = nullptr;
      fb.f[q] = owns_lookup(l) ? B.f_lag + l * n : nullptr;
      fb.b[q] = B.bpoly + l * n;
      fb.m[q] = B.m_counts + l * N;
      fb.den[q] = B.den + l * N;
    }
    CQ_TRY(cq_round2_prep(c, fb, (uint32_t)n, (uint32_t)N, u, beta));
  }
  if (resident) {
    CQ_TRY(resident_round2_invert());
  } else if (L) {
    // all inversions of the round in two launches (one Fermat inversion per lane dominates the latency)
    CQ_TRY(poly_batch_invert(c, B.bpoly, (uint32_t)(L * n + L * N)));  // bpoly and den are adjacent
  }
  size_t woff = 0;
  for (size_t l0 = 0; l0 < L; l0 += CQ_FOLD_BATCH) {  // a_i = m_i / (t_i + beta) and its theta-scaled copies for q_a (:247-256)
    CqAValuesBatch ab;
    ab.count = (uint32_t)std::min<size_t>(CQ_FOLD_BATCH, L - l0);
    ab.beta_inv = beta_inv;
    for (uint32_t j = 0; j < CQ_MAX_WIDTH; j++) ab.theta_pow[j] = theta_pow[j];
    for (uint32_t q = 0; q < ab.count; q++) {
      const size_t l = l0 + q;
      ab.width[q] = (uint32_t)pk->lookups[l].cols.size();
      ab.den_inv[q] = B.den + l * N;
      ab.m[q] = B.m_counts + l * N;
      ab.a[q] = B.a_val + l * N;
      ab.a_scaled[q] = B.a_scaled + woff * N;
      ab.b_values[q] = b_by_rows ? B.b_values + l * (N + 1) : nullptr;
      woff += ab.width[q];
    }
    CQ_TRY(cq_a_values_batch(c, ab, (uint32_t)N));
  }
  if (resident) {
    CQ_TRY(resident_round2_b_to_coeff());
  } else if (L) {
    CQ_TRY(lagrange_to_coeff_cols(B.bpoly, B.bpoly, L));  // f: under round 1's launch
    // b(0) of every lookup (for a(0), :318-324): on its way to the host while the round's MSMs run
    GatherArgs ga;
    ga.count = (uint32_t)L;
    for (size_t l = 0; l < L; l++) ga.src[l] = B.bpoly + l * n;
    CQ_TRY(poly_gather_scalars(c, ga, B.gather));
    CQ_HIP(c, hipMemcpyAsync(small_fr, B.gather, L * sizeof(Fr), hipMemcpyDeviceToHost, s));
  }
  return CQ_OK;
}
// The helper thread has had rounds 0 and 1 and this round's preparation to draw the random polynomial.  From
// k = 20 on that is not enough (2^25 words take ~25 ms at k = 22): then the polynomial is committed in a launch
// of its own after the round's other MSMs, which start now.
// Not done yet?  A launch of its own for the polynomial costs ~0.7 ms of GPU time; waiting costs what is left of
// the draws.  Wait while the estimate (from the chunks done so far) stays below that, give up otherwise.
// The choice is timing-dependent, so sharded ranks agree on it first (late on any rank = late on all: a rank that
// has the polynomial ready just commits it in the second launch too).  CQ_RANDOM_LATE=0/1 pins it (tests).
int ProofRun::round2_random_late(bool& random_late) {
  const char* force = getenv("CQ_RANDOM_LATE");
  const auto t0 = std::chrono::steady_clock::now();
  while (!drawer.done.load()) {
    if (force && force[0] == '1') break;
    const double waited = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (!(force && force[0] == '0') && waited > 100.0 && drawer.remaining_us() > 700.0) break;
    std::this_thread::yield();
  }
  CQ_TRY(shard_any(pk, (force && force[0] == '1') || !drawer.done.load(), random_late));
  return CQ_OK;
}
// round 2, the launch: side-stream fork, collection, transcript writes and a(0)
int ProofRun::round2_commit(bool random_late) {
  if (!random_late) CQ_TRY(finish_random_poly());
  // commitments, one batch of launches: the permutation products (permutation/prover.rs:177, written first),
  // then a, a0 (dense over the table SRS), q_a (over [qs_0|qs_1|...]), p, b0 (n-1 terms of b[1..]) and the
  // vanishing argument's random polynomial (vanishing/prover.rs:58)
  std::vector<G1Affine> r2;
  {
    std::vector<const Fr*> sc;
    std::vector<const G1Affine*> bs;
    std::vector<size_t> ln;
    // (b_by_rows: the 2 L short MSMs over this proof's bucket sums -- plain mode, no tables -- go first as one launch of
    // their own (a single kernel, msm_short_run), so that the table-mode MSMs behind them still share one; `at[i]`: where result i of the transcript's
    // order sits in the launch order)
    std::vector<size_t> at;
    for (size_t l = 0; b_by_rows && l < L; l++)
      for (size_t q = 0; q < 2; q++) { sc.push_back(B.b_values + l * (N + 1)); bs.push_back(B.b_sums + (2 * l + q) * (N + 1)); ln.push_back(N + 1); }
    for (size_t st = 0; st < S; st++) { at.push_back(sc.size()); sc.push_back(B.z + st * n); bs.push_back(pk->params->g_lagrange); ln.push_back(n); }
    for (size_t l = 0; l < PL; l++) { at.push_back(sc.size()); sc.push_back(plk_buf(l, 4)); bs.push_back(pk->params->g_lagrange); ln.push_back(n); }
    size_t woff = 0;
    for (size_t l = 0; l < L; l++) {
      const uint32_t w = (uint32_t)pk->lookups[l].cols.size();
      at.push_back(sc.size()); sc.push_back(B.a_val + l * N); bs.push_back(pk->table_cfg->g1_lagrange); ln.push_back(N);             // a
      at.push_back(sc.size()); sc.push_back(B.a_scaled + woff * N); bs.push_back(pk->qs_concat[l]); ln.push_back((size_t)w * N);      // q_a
      at.push_back(sc.size()); sc.push_back(B.a_val + l * N); bs.push_back(pk->table_cfg->g_lagrange_opening_at_0); ln.push_back(N);  // a0
      if (b_by_rows) {
        at.push_back(2 * l);      // b0 (:310)
        at.push_back(2 * l + 1);  // p (:299)
      } else {
        at.push_back(sc.size()); sc.push_back(B.bpoly + l * n + 1); bs.push_back(pk->params->g); ln.push_back(n - 1);     // b0
        at.push_back(sc.size()); sc.push_back(B.bpoly + l * n + 1); bs.push_back(pk->b0_g1_bound); ln.push_back(n - 1);   // p
      }
      woff += w;
    }
    if (!random_late) { at.push_back(sc.size()); sc.push_back(B.random_poly); bs.push_back(pk->params->g); ln.push_back(n); }
    Commit r2cm;
    const uint64_t seq = c->msm_tail_seq;
    if (sums_pending) {  // the short MSMs over B.b_sums are the first thing this launch queues
      CQ_HIP(c, hipStreamWaitEvent(s, c->b_sums_done, 0));
      sums_pending = false;
    }
    CQ_TRY(r2cm.begin(pk, sc, bs, ln));
    {
      // under the launch's tail, none of it depending on y: advice -> coefficients (prover.rs:587-603, in place: the
      // Lagrange values were last read by the permutation / lookup products above) and onto the extended coset
      // (evaluation.rs:317-335), b onto the extended coset
      AuxFork fork(c);
      CQ_TRY(fork.begin(seq));
      if (A && !adv_is_coeff) CQ_TRY(lagrange_to_coeff_cols(B.adv, B.adv, A));
      if (resident) CQ_TRY(resident_b_to_coset());
      else if (L) CQ_TRY(coeff_to_extended_cols(B.bpoly, B.cosets, L));
      if (general && A) CQ_TRY(coeff_to_extended_cols(B.adv, B.adv_cosets, A));
      CQ_TRY(fork.end());
    }
    if (random_late) CQ_TRY(finish_random_poly());  // queued behind the launch above
    mark("round 2 queued");
    {
      std::vector<G1Affine> in_launch_order;
      CQ_TRY(r2cm.end(in_launch_order));
      for (size_t i : at) r2.push_back(in_launch_order[i]);
    }
    mark("round 2 commitments on the host");
    if (random_late) {
      std::vector<G1Affine> rc;
      CQ_TRY(commit_batch(pk, {B.random_poly}, {pk->params->g}, n, rc));
      r2.push_back(rc[0]);
    }
  }
  for (size_t st = 0; st < S; st++)
    if (!tr.write_point(r2[st])) return c->fail(CQ_ERR_TRANSCRIPT, "permutation product commitment is the identity");
  // z -> coefficients (permutation/prover.rs:179), in place
  if (S) CQ_TRY(lagrange_to_coeff_cols(B.z, B.z, S));
  for (size_t l = 0; l < PL; l++) {
    if (!tr.write_point(r2[S + l])) return c->fail(CQ_ERR_TRANSCRIPT, "lookup product commitment is the identity");
    // a', s', z -> coefficients (lookup/prover.rs:133, 285), in place (three consecutive vectors)
    CQ_TRY(domain_lagrange_to_coeff(dom, plk_buf(l, 2), plk_buf(l, 2), 3, n, n));
  }
  for (size_t l = 0; l < L; l++) {
    // write order :306-313: a, q_a, a0, b0, p
    for (size_t q = 0; q < 5; q++)
      if (!tr.write_point(r2[S + PL + 5 * l + q])) return c->fail(CQ_ERR_TRANSCRIPT, "a CQ round-2 commitment is the identity");
  }
  random_cm = r2[S + PL + 5 * L];
  // a(0) = (n*b(0) - (bf+1)/beta) / N   (:318-324)
  if (L) {  // the copy of b(0) was queued before the launch; r2cm.end() has drained the stream
    if (resident) CQ_TRY(resident_sum_b_at_zero());
    const Fr n_table_inv = Fr::from_u64(N).inv();
    for (size_t l = 0; l < L; l++)
      a_at_zero[l] = (small_fr[l] * Fr::from_u64(n) - Fr::from_u64(bf + 1) * beta_inv) * n_table_inv;
  }
  return CQ_OK;
}

}  // namespace prover
}  // namespace cq

// Host orchestrator: `create_proof` (halo2_proofs/src/plonk/prover.rs:51-779) with the sub-arguments
// of plonk/static_lookup/prover.rs, plonk/permutation/prover.rs, plonk/vanishing/prover.rs,
// plonk/evaluation.rs:285-551 and poly/kzg/multiopen/gwc/prover.rs.  Everything O(n) runs on the GPU
// (polynomials never leave HBM); the host keeps the Fiat-Shamir transcript (transcript.rs:170-241),
// draws the blinding scalars from the caller's RNG in the reference's order, folds MSM window sums
// and normalises the handful of commitment points.  Call order, RNG order and transcript order are
// the contract: the proof bytes equal the reference's for
// the same (pk, witness, RNG stream).
//
// Scope: one circuit with advice / fixed / instance columns, custom gates (postfix programs, plonk.hip), the
// permutation argument, static (CQ) lookups whose inputs are arbitrary expressions, legacy plookup-style lookups
// (grand product and the sort of `permute_expression_pair` on the GPU, lksort.hip), multi-phase circuits with user
// challenges (cq_create_proof_phases), ProverGWC or ProverSHPLONK.  One deliberate omission:
// evaluation.rs:317-335 transforms every advice / instance polynomial to the extended coset even when no term
// reads them (a CQ-only circuit); that dead work is skipped.
//
// This file: create_proof_dev and ProofRun's set-up, instance and advice stages.  The other stages are in prover_lookup.hip,
// prover_quotient.hip and prover_open.hip, resident column sharding in prover_resident.hip; prover_run.hpp is the map.
#include "prover_run.hpp"

namespace cq {
namespace prover {

ProofRun::ProofRun(cq_pk* pk_, cq_rng_next_u64 rng_next, void* rng_state) : pk(pk_), rng{rng_next, rng_state, pk_->rng_fill, &pk_->ctx->pool()} {
  resident_init();
}
// an error return between the fork and round 2's join: the side launch reads the arena and writes its workspace, both of
// which the next proof reuses, so it has finished before this proof's frame goes
ProofRun::~ProofRun() {
  if (sums_pending) hipStreamSynchronize(c->aux_stream);
}

// Column sharding (cq_pk_set_column_sharding): a batch of independent column transforms is split
// between the ranks by owner -- contiguous ranges of columns, cq::shard_range -- and every rank's output columns are
// broadcast from their owner on the stream the transform ran on (one grouped RCCL launch).  Transforms chained on the
// same batch (coefficients, then the coset of the same columns) read what their own rank wrote, so they need not
// wait for the exchange.  Unsharded, or with fewer than two columns: the plain call.
int ProofRun::sharded_transform(bool to_extended, const Fr* in, Fr* out, uint32_t batch) {
  const size_t in_stride = n, out_stride = to_extended ? ext : n;
  auto run = [&](size_t first, size_t count) -> int {
    if (!count) return CQ_OK;
    return to_extended ? domain_coeff_to_extended(dom, in + first * in_stride, out + first * out_stride, (uint32_t)count, in_stride, out_stride)
                       : domain_lagrange_to_coeff(dom, in + first * in_stride, out + first * out_stride, (uint32_t)count, in_stride, out_stride);
  };
  if (!shard_columns_enabled(pk) || (batch < 2 && !pk->shard_single)) return run(0, batch);
  size_t lo, hi;
  shard_range(batch, pk->shard_rank, pk->shard_world, lo, hi);
  CQ_TRY(run(lo, hi - lo));
  std::vector<BcastPart> parts;
  for (uint32_t r = 0; r < pk->shard_world; r++) {
    shard_range(batch, r, pk->shard_world, lo, hi);
    if (hi > lo) parts.push_back({out + lo * out_stride, (hi - lo) * out_stride * sizeof(Fr), r});
  }
  return shard_bcast_parts(pk, parts.data(), parts.size(), c->stream);
}

// joins the helper, orders the main stream after the uploads, words -> field elements
int ProofRun::finish_random_poly() {
  if (drawer.join() != 0) return c->fail(CQ_ERR_HIP, "random polynomial upload failed");
  CQ_HIP(c, hipStreamWaitEvent(s, c->copy_done, 0));
  return poly_from_u512(c, B.rng_dev, (uint32_t)n, B.random_poly);
}

// The same launches on the side stream, queued right after the main-stream launch they run beside (`seq_before`: as for
// AuxFork): ordered after that launch's accumulate kernel, hence after cq_round1, which wrote the indices, and when the
// main stream is down to its latency-bound tail.  They go in front of the transforms AuxFork puts on that stream.
int ProofRun::fork_bucket_sums(uint64_t seq_before) {
  if (!sums_side) return CQ_OK;
  AuxFork fork(c);
  CQ_TRY(fork.begin(seq_before));
  sums_pending = true;
  CQ_TRY(bucket_sum_launches());
  CQ_HIP(c, hipEventRecord(c->b_sums_done, c->aux_stream));
  return fork.end();
}

// ---- set-up that can fail on this rank alone (allocations: arena, pinned staging, streams, twiddle tables) comes first,
//      and a sharded proof agrees on its outcome before anything else is exchanged: a rank that cannot start says so in
//      a one-word all-gather and every rank returns an error, instead of the others waiting in the first collective of a
//      proof one of them never joins.  (A failure later on one rank alone -- the MSM workspace, a HIP error -- aborts that
//      rank's communicator, and its peers' waits time out: capi_cq.hip, comm.hip.)
int ProofRun::setup() {
  void* arena_v = nullptr;
  auto allocate = [&]() -> int {
    CQ_TRY(c->ensure_scratch(Scratch::ProverArena, prover_arena_elems(pk) * sizeof(Fr), &arena_v));
    CQ_TRY(c->ensure_pinned_small(&small_v));
    CQ_TRY(c->ensure_pinned((size_t)64 * n + A * (n - u) * sizeof(Fr) + 64, &pin));
    CQ_TRY(c->ensure_aux_stream());
    CQ_TRY(c->ensure_copy_stream());
    if (resident) CQ_TRY(resident_reserve_staging());  // where received slices land
    int trc = CQ_OK;
    if (!c->tables_for(dom->k, dom->omega_inv, &trc) || !c->tables_for(dom->extended_k, dom->extended_omega, &trc)) return trc;
    return CQ_OK;
  };
  const int setup_rc = getenv("CQ_TEST_FAIL_SETUP") && atoi(getenv("CQ_TEST_FAIL_SETUP")) == (int)pk->shard_rank + 1
                           ? c->fail(CQ_ERR_HIP, "set-up failure injected by CQ_TEST_FAIL_SETUP") : allocate();
  if (pk->sharded()) {
    bool any = false;
    const std::string mine = c->err;
    CQ_TRY(shard_any(pk, setup_rc != CQ_OK, any));
    if (any) return setup_rc != CQ_OK ? c->fail(setup_rc, mine) : c->fail(CQ_ERR_INTERNAL, "sharded proof: another rank could not set up its proof (allocation failure there)");
  } else if (setup_rc != CQ_OK) {
    return setup_rc;
  }
  Arena ar{(Fr*)arena_v};
  carve(pk, ar, B);
  adv_poly = early_adv ? B.adv_coeff : B.adv;
  herr = (volatile uint32_t*)small_v;
  small_fr = (Fr*)((char*)small_v + 64);
  // side stream: drain whatever an aborted proof may have left there (its NTTs find their twiddle tables built: set-up above)
  if (c->aux_pending) {
    CQ_HIP(c, hipStreamSynchronize(c->aux_stream));
    c->aux_pending = false;
  }
  return CQ_OK;
}

// ---- instance columns (prover.rs:100-131), absorbed as scalars in phase 0 (:305-312) ---------------
int ProofRun::absorb_instances(const uint64_t* const* instances, const size_t* instance_lens) {
  if (!I) return CQ_OK;
  CQ_HIP(c, hipMemsetAsync(B.inst_lag, 0, I * n * sizeof(Fr), s));
  for (size_t i = 0; i < I; i++) {
    if (instance_lens[i] > u) return c->fail(CQ_ERR_ARG, "Error::InstanceTooLarge");  // :108-110
    if (instance_lens[i])
      CQ_HIP(c, hipMemcpyAsync(B.inst_lag + i * n, instances[i], instance_lens[i] * sizeof(Fr), hipMemcpyHostToDevice, s));
  }
  CQ_TRY(domain_lagrange_to_coeff(dom, B.inst_lag, B.inst_coeff, (uint32_t)I, n, n));
  for (size_t i = 0; i < I; i++)
    for (size_t r = 0; r < instance_lens[i]; r++) tr.common_scalar(Fr::from_limbs64(instances[i] + 4 * r));
  return CQ_OK;
}

// ---- advice, phase by phase (`next_phase`, prover.rs:299-391; the synthesis loop :436-463): copy the phase's
//      columns in, blind rows u..n (:346-350), one unused blind per column (:352-355), commit, squeeze the phase's
//      challenges ----------------------------------------------------------------------------------------------
int ProofRun::advice_phase(uint32_t phase, const uint64_t* const* advice_dev, cq_phase_fn phase_fn, void* phase_user) {
  const bool last_phase = phase + 1 == pk->num_phases;
  std::vector<size_t> cols;
  for (size_t a = 0; a < A; a++)
    if (phase_of(a) == phase) cols.push_back(a);
  if (phase > 0) {
    // the caller computes this phase's witness from the challenges of the earlier phases
    std::vector<uint64_t> ch(4 * std::max<size_t>(NC, 1), 0);
    for (size_t i = 0; i < NC; i++) user_challenges[i].to_limbs64(ch.data() + 4 * i);
    CQ_TRY(c->wait(s));
    if (!phase_fn || phase_fn(phase_user, phase, ch.data(), (uint64_t* const*)advice_dev) != 0)
      return c->fail(CQ_ERR_ARG, "create_proof: the phase callback failed");
  }
  const size_t AC = cols.size();
  std::vector<Fr> tails(AC * (n - u));
  for (size_t j = 0; j < AC; j++)
    for (size_t r = 0; r < n - u; r++) tails[j * (n - u) + r] = rng.fr();
  for (size_t j = 0; j < AC; j++) (void)rng.fr();
  // pinned staging: [0, 64 n) the random polynomial's words (filled by the helper thread from the last phase on),
  // behind it this phase's blinding rows -- no part is reused within a proof, so nothing waits for a copy to finish
  Fr* pin_tails = (Fr*)((char*)pin + (size_t)64 * n);
  if (phase > 0) CQ_TRY(c->wait(s));  // the previous phase's upload out of the same bytes has been consumed
  memcpy(pin_tails, tails.data(), tails.size() * sizeof(Fr));
  if (AC) CQ_HIP(c, hipMemcpyAsync(B.tails, pin_tails, tails.size() * sizeof(Fr), hipMemcpyHostToDevice, s));
  for (size_t off = 0; off < AC; off += ADVICE_FILL_MAX) {  // rows [0, u) from the caller's columns, [u, n) the blinding rows
    AdviceFillArgs fa;
    fa.count = (uint32_t)std::min<size_t>(ADVICE_FILL_MAX, AC - off);
    for (uint32_t j = 0; j < fa.count; j++) {
      fa.src[j] = (const Fr*)advice_dev[cols[off + j]];
      fa.dst[j] = B.adv + cols[off + j] * n;
    }
    CQ_TRY(poly_advice_fill(c, fa, B.tails + off * (n - u), (uint32_t)n, u));
  }
  // commit_lagrange per column (:356-360): enqueue now, collect after the host work below
  std::vector<const Fr*> sc(AC);
  std::vector<const G1Affine*> bs(AC, pk->params->g_lagrange);
  std::vector<size_t> ln(AC, n);
  for (size_t j = 0; j < AC; j++) sc[j] = B.adv + cols[j] * n;
  if (early_m) {  // m_cm (:167-172, as a dense MSM over the table SRS) rides along
    CQ_TRY(count_multiplicities());
    for (size_t l = 0; l < L; l++) { sc.push_back(B.m_fr + l * N); bs.push_back(pk->table_cfg->g1_lagrange); ln.push_back(N); }
  }
  Commit adv_cm;
  const uint64_t seq_adv = c->msm_tail_seq;
  if (!sc.empty()) CQ_TRY(adv_cm.begin(pk, sc, bs, ln));
  if (early_m) CQ_TRY(fork_bucket_sums(seq_adv));
  if (early_adv) {
    // advice -> coefficients (prover.rs:587-603) on the side stream, behind this launch's accumulate kernel: it runs
    // under the launch's tail and the host's round trip for theta, when the GPU has little else to do -- after theta
    // it would compete with the critical path from beta to round 2's launch (round 3: -0.3 ms at k = 18)
    AuxFork fork(c);
    CQ_TRY(fork.begin(seq_adv));
    if (resident) CQ_TRY(resident_advice_to_coeff());
    else CQ_TRY(lagrange_to_coeff_cols(B.adv, adv_poly, A));
    CQ_TRY(fork.end());
    adv_is_coeff = true;
  }
  if (last_phase) {
    // The next draws from the RNG are, per permutation set, `bf` blinding rows of z and one blind
    // (permutation/prover.rs:169-175), then the vanishing argument's n coefficients + 1 blind
    // (vanishing/prover.rs:51-55): the CQ rounds in between draw nothing, so taking them now keeps the
    // stream order, overlaps the host-side draws with the advice MSMs, and lets the random
    // polynomial's commitment ride along with round 2's launch.
    // legacy lookups, commit_permuted (lookup/prover.rs:491-494, 133-145): bf+1 rows of a', bf+1 rows of s', two blinds
    for (size_t l = 0; l < PL; l++) {
      for (uint32_t r = 0; r < 2 * (bf + 1); r++) plk_tails[l * 2 * (bf + 1) + r] = rng.fr();
      (void)rng.fr();
      (void)rng.fr();
    }
    for (size_t st = 0; st < S; st++) {
      for (uint32_t r = 0; r < bf; r++) z_tails[st * bf + r] = rng.fr();
      (void)rng.fr();  // permutation_product_blind
    }
    // legacy lookups, commit_product (:237, 283): bf rows of z, one blind
    for (size_t l = 0; l < PL; l++) {
      for (uint32_t r = 0; r < bf; r++) plkz_tails[l * bf + r] = rng.fr();
      (void)rng.fr();
    }
    // the random polynomial's words: drawn and uploaded by the helper thread from here on (see RandomPolyDrawer)
    drawer.start(c, &rng, (uint64_t*)pin, B.rng_dev, 8 * n);
  }
  // batch_normalize (:363-366), write (:370-374)
  mark("advice launch queued");
  if (!sc.empty()) {
    std::vector<G1Affine> pts;
    CQ_TRY(adv_cm.end(pts));
    mark("advice commitments on the host");
    if (early_m) CQ_TRY(lookup_error());
    for (size_t j = 0; j < AC; j++)
      if (!tr.write_point(pts[j])) return c->fail(CQ_ERR_TRANSCRIPT, "advice commitment is the identity");
    for (size_t j = 0; j < AC; j++) advice_commitments[cols[j]] = pts[j];
    if (early_m)
      for (size_t l = 0; l < L; l++) m_commitments[l] = pts[AC + l];
  } else {
    CQ_TRY(c->wait(s));
  }
  for (size_t i = 0; i < NC; i++)  // :383-389
    if (pk->challenge_phase[i] == phase) user_challenges[i] = tr.squeeze();
  return CQ_OK;
}
int ProofRun::advice_phases(const uint64_t* const* advice_dev, cq_phase_fn phase_fn, void* phase_user) {
  for (uint32_t phase = 0; phase < pk->num_phases; phase++) CQ_TRY(advice_phase(phase, advice_dev, phase_fn, phase_user));
  if (NC) CQ_HIP(c, hipMemcpyAsync(B.challenges, user_challenges.data(), NC * sizeof(Fr), hipMemcpyHostToDevice, s));
  return CQ_OK;
}

}  // namespace prover

using namespace prover;

size_t prover_arena_elems(const cq_pk* pk) {
  Arena ar{nullptr};
  Buffers b;
  carve(pk, ar, b);
  return ar.used + 1024;
}

int create_proof_dev(cq_pk* pk, const uint64_t* const* advice_dev, const uint64_t* const* instances,
                     const size_t* instance_lens, cq_phase_fn phase_fn, void* phase_user, cq_rng_next_u64 rng_next,
                     void* rng_state, std::vector<uint8_t>& proof_out) {
  ProofRun run(pk, rng_next, rng_state);
  Transcript& tr = run.tr;
  cq_ctx* c = pk->ctx;
  CQ_TRY(run.setup());
  tr.common_scalar(pk->vk_repr);  // prover.rs:85 -- vk.hash_into(transcript)
  CQ_TRY(run.absorb_instances(instances, instance_lens));
  CQ_TRY(run.advice_phases(advice_dev, phase_fn, phase_user));
  run.theta = tr.squeeze();  // :472
  run.mark("theta");
  CQ_TRY(run.legacy_commit_permuted());
  CQ_TRY(run.cq_round1());
  run.mark("round 1 written");
  run.beta = tr.squeeze();   // prover.rs:529
  run.gamma = tr.squeeze();  // :532
  run.beta_inv = run.beta.inv();
  CQ_TRY(run.permutation_commit());
  CQ_TRY(run.legacy_commit_product());
  CQ_TRY(run.cq_round2());
  // ---- vanishing::Argument::commit (vanishing/prover.rs:37-65): drawn and committed in round 2 ---------
  if (!tr.write_point(run.random_cm)) return c->fail(CQ_ERR_TRANSCRIPT, "random poly commitment is the identity");
  run.y = tr.squeeze();  // prover.rs:584
  run.mark("y");
  // advice polys (lagrange_to_coeff, :587-603) and the cosets of advice / instance / b / f were computed on the side
  // stream under the round-1 and round-2 launches
  CQ_TRY(join_aux(c));
  CQ_TRY(run.evaluate_h());
  CQ_TRY(run.construct_h());
  run.x = tr.squeeze();  // prover.rs:629
  run.mark("x");
  run.xn = run.x.pow_u64(run.n);
  CQ_TRY(run.evaluate_and_write());
  if (pk->opener == CQ_OPENER_SHPLONK) {
    CQ_TRY(run.open_shplonk());
  } else {
    CQ_TRY(run.open_gwc());
    run.mark("done");
  }
  proof_out.swap(tr.proof);
  return CQ_OK;
}

}  // namespace cq

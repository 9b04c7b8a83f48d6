// Internal interface of the host orchestrator's translation units: what two or more of them share.
//   prover.hip           create_proof_dev, ProofRun's set-up, instance and advice stages
//   prover_support.hip   commitments of a round (Commit), RNG adapter, arena layout, lincomb / eval batches, the random
//                        polynomial's helper thread
//   prover_lookup.hip    CQ rounds 1 and 2, the legacy lookups' permuted columns and products
//   prover_quotient.hip  permutation products, evaluate_h, the quotient's pieces
//   prover_open.hip      evaluations, ProverGWC and ProverSHPLONK
//   prover_stages.hip    the stages as stand-alone calls (stage_*, prover.hpp)
//   prover_resident.hip  resident column sharding: every ProofRun::resident_* method
// prover.hpp is the interface the rest of the library sees.
#pragma once
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>
#include "blake2b.hpp"
#include "comm.hpp"
#include "cq.hpp"
#include "ctx.hpp"
#include "msm.hpp"
#include "plonk.hpp"
#include "prover.hpp"
#include "glv.hpp"
#include "xoshiro.hpp"

namespace cq {
namespace prover {

struct Transcript {
  Blake2b st;
  std::vector<uint8_t> proof;
  Transcript() { st.init(64, "Halo2-Transcript"); }
  void common_scalar(const Fr& s) {
    const uint8_t tag = 2;
    st.update(&tag, 1);
    U256 c = s.to_canonical();
    st.update((const uint8_t*)c.l, 32);
  }
  // transcript.rs:221-233; identity is an error
  bool common_point(const G1Affine& p) {
    if (p.is_identity()) return false;
    const uint8_t tag = 1;
    st.update(&tag, 1);
    U256 x = p.x.to_canonical(), y = p.y.to_canonical();
    st.update((const uint8_t*)x.l, 32);
    st.update((const uint8_t*)y.l, 32);
    return true;
  }
  bool write_point(const G1Affine& p) {
    if (!common_point(p)) return false;
    U256 x = p.x.to_canonical(), y = p.y.to_canonical();
    uint8_t b[32];
    memcpy(b, x.l, 32);
    b[31] |= (uint8_t)((y.l[0] & 1) << 7);  // derive/curve.rs:635-646
    proof.insert(proof.end(), b, b + 32);
    return true;
  }
  void write_scalar(const Fr& s) {
    common_scalar(s);
    U256 c = s.to_canonical();
    const uint8_t* b = (const uint8_t*)c.l;
    proof.insert(proof.end(), b, b + 32);
  }
  Fr squeeze() {
    const uint8_t tag = 0;
    st.update(&tag, 1);
    uint8_t out[64];
    st.finalize_clone(out);
    uint64_t w[8];
    memcpy(w, out, 64);
    return Fr::from_u512(w);  // from_bytes_wide (transcript.rs:300-309)
  }
};

struct Rng {
  cq_rng_next_u64 next;
  void* state;
  cq_rng_fill_fn bulk = nullptr;  // the caller's own bulk form (cq_pk_set_rng_fill)
  HostPool* pool = nullptr;       // the context's worker threads
  // Fr::random (bn256/fr.rs:159-170): eight next_u64, low limb first
  void words(uint64_t* w8) {
    for (int i = 0; i < 8; i++) w8[i] = next(state);
  }
  Fr fr() {
    uint64_t w[8];
    words(w);
    return Fr::from_u512(w);
  }
  // `count` consecutive draws; the library's own generators are recognised and run inline (the indirect
  // call per u64 costs more than the generator: 2^21 draws per k=18 proof)
  void fill(uint64_t* dst, size_t count);
};

// CQ_TRACE_HOST is set: host milestones and the phases of Commit::end go to stderr (development aid; read once)
bool host_trace_enabled();

// Commitments of one transcript round.  begin() enqueues the (possibly sharded) MSMs, end() waits,
// exchanges partial sums between ranks when sharded, and normalises (batch_normalize).
struct Commit {
  const cq_pk* pk;
  MsmPending pend;
  size_t count = 0;
  int begin(const cq_pk* pk_, const std::vector<const Fr*>& scalars, const std::vector<const G1Affine*>& bases,
            const std::vector<size_t>& lens);
  int end(std::vector<G1Affine>& out);
};
int commit_batch_v(const cq_pk* pk, const std::vector<const Fr*>& scalars, const std::vector<const G1Affine*>& bases,
                   const std::vector<size_t>& lens, std::vector<G1Affine>& out);
int commit_batch(const cq_pk* pk, const std::vector<const Fr*>& scalars, const std::vector<const G1Affine*>& bases, size_t len,
                 std::vector<G1Affine>& out);

// A decision that changes the STRUCTURE of a round (how many launches, hence how many collectives and of what size) must
// come out the same on every rank: true everywhere iff `flag` is set on any rank (one 8-byte all-gather).
int shard_any(const cq_pk* pk, bool flag, bool& out);

// Work for the side stream (ctx.hpp): between begin() and end() every library call that enqueues on `c->stream`
// lands on the low-priority stream instead, ordered after the accumulate kernel of the MSM launch queued last (all
// earlier kernels of the main stream are complete by then, and what remains of the MSM only touches its own
// workspace).  join_aux() makes the main stream wait for it.  The destructor restores the context on an error path.
// (An MSM launched between begin() and end() -- ProofRun::fork_bucket_sums -- leaves msm_tail_event and msm_tail_seq alone,
// msm.hip: the next fork's begin(seq) still finds the main-stream launch it was sampled for.)
struct AuxFork {
  cq_ctx* c;
  hipStream_t main = nullptr;
  bool active = false;
  explicit AuxFork(cq_ctx* c_) : c(c_) {}
  // `seq_before`: c->msm_tail_seq sampled before the MSMs were queued
  int begin(uint64_t seq_before) {
    if (c->msm_tail_seq == seq_before) CQ_HIP(c, hipEventRecord(c->msm_tail_event, c->stream));  // no launch: plain ordering
    CQ_HIP(c, hipStreamWaitEvent(c->aux_stream, c->msm_tail_event, 0));
    main = c->stream;
    c->stream = c->aux_stream;
    active = true;
    return CQ_OK;
  }
  int end() {
    if (!active) return CQ_OK;
    restore();
    c->aux_pending = true;
    CQ_HIP(c, hipEventRecord(c->aux_done, c->aux_stream));
    return CQ_OK;
  }
  void restore() {
    c->stream = main;
    active = false;
  }
  ~AuxFork() {
    if (active) {
      restore();
      hipStreamSynchronize(c->aux_stream);
    }
  }
};
inline int join_aux(cq_ctx* c) {
  if (!c->aux_pending) return CQ_OK;
  c->aux_pending = false;
  CQ_HIP(c, hipStreamWaitEvent(c->stream, c->aux_done, 0));
  return CQ_OK;
}

// Proof-lifetime device buffers, carved from one arena (scratch slot 6).  With base == nullptr the same
// code only counts elements.
struct Arena {
  Fr* base;
  size_t used = 0;
  Fr* take(size_t elems) {
    Fr* p = base ? base + used : nullptr;
    used += elems;
    return p;
  }
};
struct Buffers {
  Fr *adv, *adv_coeff, *inst_lag, *inst_coeff, *f_lag, *f_coeff, *bpoly, *random_poly, *z, *mv, *cosets, *adv_cosets, *inst_cosets,
      *z_cosets, *lk_inputs, *plk, *plk_cosets, *h_ext, *h_coeff, *gwc_batch, *gwc_wit, *shplonk, *den, *a_val, *m_fr, *a_scaled;
  Fr* challenges;  // user challenges (Expression::Challenge), uploaded as the phases complete
  // b's commitments from per-table-row sums (round 2): the N + 1 values b takes, per lookup; the bucket sums -- per lookup
  // two arrays of N + 1 affine points (64 B = 2 Fr each) -- that a launch before theta leaves there
  // and, per lookup, the n bucket indices cq_round1 writes for the launch that forms the sums.  The indices have a region of
  // their own, not b's then unused buffer: the launch runs on a side stream beside the main stream's work up to round 2,
  // whose preparation writes b -- with their own region the main stream never has to wait for the launch's last reader
  Fr* b_values;
  G1Affine* b_sums;
  uint32_t* b_index;
  Fr *tails, *gather;  // blinding rows of a phase's advice columns (staging); scalars on their way to the host
  uint64_t* rng_dev;
  uint32_t *m_counts, *err_dev;
};
bool early_advice_polys(const cq_pk* pk);
void carve(const cq_pk* pk, Arena& ar, Buffers& b);

// sum_i coeff_i * p_i - sub_const, any number of terms (LINCOMB_MAX per launch; later launches fold the
// partial result back in as one more term)
struct Term {
  const Fr* p;
  uint32_t len;
  Fr coeff;
};
int lincomb_many(cq_ctx* c, const std::vector<Term>& terms, const Fr& sub_const, uint32_t n, Fr* out);
int eval_many(cq_ctx* c, const std::vector<const Fr*>& ps, const std::vector<uint32_t>& ls, const Fr& z, Fr* out);

// One opening query.  Every polynomial opened by the proof is listed in the order ProverGWC receives the queries; h is
// opened but its value is derived (vanishing/prover.rs:131-153).
struct Query {
  const Fr* p;
  uint32_t len;
  int32_t rot;
  int h_piece;  // -1, or the index of an h piece (folded into one query with coefficient xn^i)
  Fr eval;
  uint32_t pt = 0;  // the query's point, as an index into the distinct points in first-seen order: what the openers go by
};

// ---- The stages a caller may also run on their own (cq_permutation_commit_dev, cq_lookup_commit_product_dev,
//      cq_evaluate_h_dev, cq_multiopen_dev; prover_stages.hip): one implementation each, which ProofRun's methods and
//      the stand-alone entry points both call.  They take device pointers and challenges, enqueue on the context's stream,
//      and know nothing of the proof's arena, transcript or RNG (prover_quotient.hip, prover_open.hip). -----------------
struct HTermsArgs {
  const Fr *adv_cosets, *inst_cosets, *z_cosets;  // num_advice / num_instance / sets x ext
  const Fr* challenges;                           // device: user challenges
  const Fr* const* plk_polys;                     // per legacy lookup: a', s', z, three consecutive vectors of n coefficients
  Fr* plk_cosets;                                 // legacy lookups x 5 x ext, written here
  Fr beta, gamma, theta, y;
};
int perm_products(const cq_pk* pk, const Fr* const* cols, const Fr& beta, const Fr& gamma, const Fr* z_tails, Fr* mv, Fr* z);
int lookup_product(cq_ctx* c, const Fr* cin, const Fr* ctab, const Fr* perm_in, const Fr* perm_tab, const Fr& beta, const Fr& gamma,
                   const Fr* tails, uint32_t n, uint32_t bf, Fr* z);
int h_terms(const cq_pk* pk, const HTermsArgs& t, Fr* h_ext);

// The multi-open argument over a list of queries.  Polynomials may be shorter than n: every combination below is one
// poly_lincomb launch (lincomb_kernel: one lane per coefficient, a term contributes only where the lane is below its
// own length), so mixed lengths need no kernel of their own.  The transcript is reached through two hooks, the
// proof's own or a caller's callbacks; both return CQ_OK or the error to pass on.
struct OpenTranscript {
  std::function<int(Fr&)> squeeze;
  std::function<int(const G1Affine&, const char* what)> write_point;  // `what` names the point should it be the identity
};
struct OpenJob {
  const cq_pk* pk;
  const std::vector<Query>* qs;    // evaluations filled in
  const std::vector<Fr>* points;   // the distinct points, first-seen order (Query::pt)
  const std::vector<size_t>* q_h;  // the queries that are pieces of h (none outside a proof); they share one power of v
  Fr xn;                           // x^n, the pieces' weight
  Fr *gwc_batch, *gwc_wit;         // GWC: points x n each
  Fr* shplonk;                     // SHPLONK: 5 n + 64 * 8 (h, two division buffers, h_x, l_x, low-degree remainders)
  OpenTranscript tr;
  // GWC, optional: forms point g's witness polynomial from the combination's terms in place of lincomb + kate_division
  // (resident sharding, where no rank holds every term)
  std::function<int(size_t g, const std::vector<Term>& terms, const Fr& eval_batch, Fr* batch, Fr* wit)> witness;
};
int open_gwc_queries(OpenJob& j);
int open_shplonk_queries(OpenJob& j);

// The vanishing argument's random polynomial (vanishing/prover.rs:51-55: n field elements = 8n words, then one
// blind) is the bulk of the RNG stream -- 2^21 words at k = 18, 2^25 (268 MB) at k = 22, more host time than the
// GPU needs for the advice and round-1 commitments together.  Every draw that precedes it in stream order is made
// up front by the main thread; the words themselves are drawn by a helper thread, chunk by chunk, each chunk
// uploaded on the side stream as soon as it is drawn, while the main thread runs rounds 0 and 1.  The main thread
// does not touch the RNG again before it has joined the helper (just before round 2 commits the polynomial).
struct RandomPolyDrawer {
  std::thread th;
  bool running = false;
  std::atomic<bool> done{false};
  std::atomic<uint32_t> chunks_done{0};
  uint32_t chunks_total = 1;
  std::chrono::steady_clock::time_point t_start;
  hipError_t err = hipSuccess;
  // estimated time to completion in microseconds (from the progress so far); 0 when done
  double remaining_us() const {
    if (done.load()) return 0.0;
    const double el = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_start).count();
    const uint32_t d = chunks_done.load();
    return d ? el * (double)(chunks_total - d + 1) / d : 1e9;  // +1: the last upload's event
  }
  void start(cq_ctx* c, Rng* rng, uint64_t* pin, uint64_t* dev, size_t words);
  int join();
  ~RandomPolyDrawer() {
    if (running) th.join();
  }
};

// One proof.  `create_proof_dev` calls the stages below in the reference's order (plonk/prover.rs).  The members are what
// crosses a stage boundary -- what one stage leaves behind for a later one; everything else is a local of its stage.
struct ProofRun {
  cq_pk* const pk;
  cq_ctx* const c = pk->ctx;
  cq_domain* const dom = pk->domain;
  const hipStream_t s = c->stream;
  const uint32_t k = pk->k;
  const size_t n = (size_t)1 << k, ext = dom->ext();
  const uint32_t bf = pk->bf, u = pk->u;
  const size_t L = pk->lookups.size(), A = pk->num_advice, I = pk->num_instance;
  const size_t N = pk->table_cfg ? pk->table_cfg->N : 0;
  const size_t S = pk->perm_sets(), PC = pk->perm_columns.size(), chunk_len = pk->cs_degree - 2;
  const size_t PL = pk->legacy.size(), NC = pk->challenge_phase.size(), pieces = dom->quotient_poly_degree;
  const bool general = pk->general();
  // [m] is committed in the advice launch (see count_multiplicities); the advice polynomials get a buffer of their own
  const bool early_m = L > 0 && pk->num_phases == 1 && pk->challenge_phase.empty();
  const bool early_adv = early_advice_polys(pk);
  // [b_0] and [p] of every lookup as MSMs of N + 1 terms over per-table-row sums of the key's per-row bases (cq.hpp:
  // b_row_bases) instead of n - 1 terms over the SRS: b takes one value per table row looked up and one on the blinding
  // rows.  Which rows share a value is known from the witness alone, so the sums are formed where m is counted, ahead of
  // theta and beta.  Sharded keys commit slices of b's coefficients by point range and keep that path.
  // A launch the MSM engine cannot plan (entry bound, workspace cap) leaves the coefficient path too.
  const bool b_by_rows = L > 0 && !pk->sharded() && pk->b_row_bases[0] != nullptr &&
                         msm_bucket_sums_fit((uint32_t)n, (uint32_t)std::min<size_t>(2 * L, MSM_MAX_BATCH));
  // Round 2 is the first reader of those sums, so their launch does not stand in front of the launch that commits [m]
  // (the advice launch with `early_m`, round 1's otherwise) but runs beside it on a side stream, from that launch's
  // accumulate kernel on (fork_bucket_sums); round2_commit joins it.  CQ_BUCKET_SUMS_SIDE=0 keeps it on the main stream,
  // in front (the A/B of profiles/r16_bucket_sums_side_ab.txt, tests); read once per proof.
  const bool sums_side = b_by_rows && side_switch();
  bool sums_pending = false;  // the side launch is queued, and nothing has made the main stream or the host wait for it yet
  static bool side_switch() {
    const char* e = getenv("CQ_BUCKET_SUMS_SIDE");
    return !(e && e[0] == '0');
  }

  // Resident column sharding (cq_pk_set_resident_sharding; DESIGN.md, multi-GPU): for the CQ-shaped circuits of the
  // BASELINE configs -- advice columns, static lookups on plain advice inputs, one phase, ProverGWC -- a transformed
  // column stays on its owner and only slices travel.  Ownership: contiguous ranges (shard_range) of the lookups and of
  // the advice columns; consumers by point range, as the MSMs are cut.  Where the proof departs from the replicated flow
  // a stage hands over to one of the resident_* methods at the end of this struct (prover_resident.hip); every rank
  // still derives the same transcript.
  bool resident = false;  // resident_init()
  const uint32_t SW = pk->shard_world, me = pk->shard_rank;
  size_t lk_lo = 0, lk_hi = L, adv_lo = 0, adv_hi = A;  // the lookups / advice columns this rank owns
  size_t lk_cnt = L;
  // resident: staging for the slices a rank receives -- per exchange at most one slice from every rank (or every owner
  // and piece), plus the rank's own range of the opening's batch polynomial with its two edge elements
  const size_t res_slice_max = (n + pk->shard_world - 1) / pk->shard_world + 1;
  const size_t res_stage_elems = (size_t)pk->shard_world * res_slice_max * (pk->cs_degree > 2 ? pk->cs_degree - 1 : 1) + res_slice_max + 64;
  void* res_stage_v = nullptr;

  Rng rng;
  Transcript tr;
  Buffers B;
  // pinned staging: `pin` holds the random polynomial's words and the advice blinding rows; `small_v` the lookup error
  // flag (`herr`), the legacy permute's status words and the scalars read back (`small_fr`: b(0), z values)
  void *pin = nullptr, *small_v = nullptr;
  volatile uint32_t* herr = nullptr;
  Fr* small_fr = nullptr;
  const std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();

  // blinding rows drawn ahead of their stages (advice_phase): permutation products, legacy permuted columns / products
  std::vector<Fr> z_tails = std::vector<Fr>(S * bf), plk_tails = std::vector<Fr>(PL * 2 * (bf + 1)), plkz_tails = std::vector<Fr>(PL * bf);
  // round 0 / 1: where each lookup input lives (Lagrange basis), the commitments later rounds and the f fold reuse
  std::vector<std::array<const Fr*, CQ_MAX_WIDTH>> lk_input = std::vector<std::array<const Fr*, CQ_MAX_WIDTH>>(L);
  std::vector<G1Affine> m_commitments = std::vector<G1Affine>(L, G1Affine::identity());
  std::vector<G1Affine> advice_commitments = std::vector<G1Affine>(A, G1Affine::identity());
  std::vector<Fr> user_challenges = std::vector<Fr>(NC, Fr::zero());
  Fr* adv_poly = nullptr;     // where the advice polynomials (coefficient form) live
  bool adv_is_coeff = false;  // the advice columns have been transformed (on the side stream, by whichever round came first)
  // challenges, squeezed by create_proof_dev between the stages
  Fr theta, beta, gamma, beta_inv, y, x, xn;
  Fr theta_pow[CQ_MAX_WIDTH];  // powers of theta for the folds of this proof (theta^0 .. theta^(CQ_MAX_WIDTH - 1))
  // round 2 -> evaluations / the vanishing argument
  std::vector<Fr> a_at_zero = std::vector<Fr>(L);
  G1Affine random_cm = G1Affine::identity();
  // evaluate_and_write -> the openers: the queries, the h pieces among them, the distinct rotations in first-seen order,
  // and (resident) the owner of each query with this rank's point range of a length-n vector
  std::vector<Query> qs;
  std::vector<size_t> q_h;
  std::vector<int32_t> rots;
  std::vector<Fr> points;
  std::vector<int> qowner;
  size_t my_lo = 0, my_hi = n;
  RandomPolyDrawer drawer;  // last member: joined (destroyed) before anything its thread reads goes away

  ProofRun(cq_pk* pk_, cq_rng_next_u64 rng_next, void* rng_state);
  ~ProofRun();

  // CQ_TRACE_HOST=1: microseconds since the start of the proof at the host's milestones, on stderr (development aid)
  void mark(const char* what) const {
    if (host_trace_enabled()) fprintf(stderr, "[cq host] %8.1f us  %s\n", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_start).count(), what);
  }
  uint32_t phase_of(size_t a) const { return pk->advice_phase.empty() ? 0u : pk->advice_phase[a]; }
  Fr* plk_buf(size_t l, int which) const { return B.plk + (l * 5 + which) * n; }  // 0 A, 1 S, 2 a', 3 s', 4 z
  Fr point_of(int32_t rot) const { return rot >= 0 ? x * dom->omega.pow_u64((uint64_t)rot) : x * dom->omega_inv.pow_u64((uint64_t)(-(int64_t)rot)); }  // rotate_omega (domain.rs:414-424)
  size_t add_query(const Fr* p, size_t len, int32_t rot) {  // rotations that name one point become one rotation (pk.hpp)
    qs.push_back({p, (uint32_t)len, pk->point_rotation(rot), -1, Fr::zero()});
    return qs.size() - 1;
  }
  // this rank holds f_l and b_l of lookup l: every lookup in the replicated flow, the owned range under resident sharding
  bool owns_lookup(size_t l) const { return l >= lk_lo && l < lk_hi; }

  // prover.hip
  int sharded_transform(bool to_extended, const Fr* in, Fr* out, uint32_t batch);
  int lagrange_to_coeff_cols(const Fr* in, Fr* out, size_t batch) { return sharded_transform(false, in, out, (uint32_t)batch); }
  int coeff_to_extended_cols(const Fr* in, Fr* out, size_t batch) { return sharded_transform(true, in, out, (uint32_t)batch); }
  int finish_random_poly();
  int fork_bucket_sums(uint64_t seq_before);
  int setup();
  int absorb_instances(const uint64_t* const* instances, const size_t* instance_lens);
  int advice_phase(uint32_t phase, const uint64_t* const* advice_dev, cq_phase_fn phase_fn, void* phase_user);
  int advice_phases(const uint64_t* const* advice_dev, cq_phase_fn phase_fn, void* phase_user);
  // prover_lookup.hip
  GateEvalArgs lagrange_eval_args(const uint32_t* prog, uint32_t num_polys, const Fr& fold) const;
  int lagrange_compress(const uint32_t* prog, uint32_t width, const Fr& chal, Fr* dst);
  int count_multiplicities();
  int bucket_sum_launches();
  int lookup_error();
  int legacy_commit_permuted();
  int cq_round1();
  int legacy_commit_product();
  int cq_round2();
  int round2_prepare();
  int round2_random_late(bool& random_late);
  int round2_commit(bool random_late);
  // prover_quotient.hip
  int permutation_commit();
  int evaluate_h();
  int construct_h();
  // prover_open.hip
  int evaluate_and_write();
  OpenJob open_job();
  int open_shplonk();
  int open_gwc();
  // prover_resident.hip: the resident flow's part of the stage named in each comment there
  uint32_t owner_of(size_t item, size_t count) const;
  void resident_init();
  int resident_reserve_staging();
  int resident_advice_to_coeff();
  int resident_round1_transforms();
  int resident_round2_invert();
  int resident_round2_b_to_coeff();
  int resident_b_to_coset();
  int resident_sum_b_at_zero();
  int resident_quotient(CqQuotientArgs& qa);
  int resident_collect_h();
  int resident_evaluate(const std::vector<size_t>& q_advice, const std::vector<size_t>& q_b0, const std::vector<size_t>& q_f);
  int resident_witness(size_t g, const std::vector<Term>& terms, const Fr& eval_batch, Fr* batch, Fr* wit);
};

}  // namespace prover
}  // namespace cq

// What the prover's stages lean on (prover_run.hpp): the commitments of a transcript round, the RNG adapter, the proof
// arena's layout, batched linear combinations and evaluations, and the helper thread that draws the random polynomial.
#include "prover_run.hpp"

namespace cq {
namespace prover {

namespace {

// derive/curve.rs:362-397 `batch_normalize`
void batch_normalize(const std::vector<G1Jac>& in, std::vector<G1Affine>& out) {
  out.resize(in.size());
  std::vector<Fq> pref(in.size());
  Fq acc = Fq::one();
  for (size_t i = 0; i < in.size(); i++) {
    pref[i] = acc;
    if (!in[i].is_identity()) acc = acc * in[i].z;
  }
  acc = acc.inv();
  for (size_t i = in.size(); i-- > 0;) {
    if (in[i].is_identity()) {
      out[i] = G1Affine::identity();
      continue;
    }
    Fq zi = pref[i] * acc;
    acc = acc * in[i].z;
    Fq zi2 = zi.sqr();
    out[i] = {in[i].x * zi2, in[i].y * zi2 * zi};
  }
}

G1Jac jac_from_limbs(const uint64_t* l) {
  return {Fq::from_limbs64(l), Fq::from_limbs64(l + 4), Fq::from_limbs64(l + 8)};
}

}  // namespace

bool host_trace_enabled() {
  static const bool on = getenv("CQ_TRACE_HOST") != nullptr;
  return on;
}

// `count` consecutive draws; the library's own generators are recognised and run inline (the indirect
// call per u64 costs more than the generator: 2^21 draws per k=18 proof)
void Rng::fill(uint64_t* dst, size_t count) {
  if (bulk) {
    bulk(state, dst, count);
  } else if (next == cq_xoshiro256ss_next_u64) {
    xoshiro_fill((uint64_t*)state, dst, count, 8, pool);  // several threads for long runs, the same stream (xoshiro.hpp)
  } else if (next == cq_buffer_rng_next_u64) {
    cq_buffer_rng* b = (cq_buffer_rng*)state;
    const size_t avail = b->pos < b->len ? b->len - b->pos : 0, take = std::min(avail, count);
    memcpy(dst, b->words + b->pos, take * sizeof(uint64_t));
    memset(dst + take, 0, (count - take) * sizeof(uint64_t));
    b->pos += take;
    b->overrun += count - take;  // create_proof fails on an exhausted stream (capi_cq.hip)
  } else {
    for (size_t i = 0; i < count; i++) dst[i] = next(state);
  }
}

int Commit::begin(const cq_pk* pk_, const std::vector<const Fr*>& scalars, const std::vector<const G1Affine*>& bases,
                  const std::vector<size_t>& lens) {
  pk = pk_;
  count = scalars.size();
  if (!pk->sharded()) return msm_multi_begin(pk->ctx, scalars.data(), bases.data(), lens.data(), count, pend);
  std::vector<const Fr*> sc(count);
  std::vector<const G1Affine*> bs(count);
  std::vector<size_t> ln(count);
  for (size_t j = 0; j < count; j++) {
    size_t lo, hi;
    shard_range(lens[j], pk->shard_rank, pk->shard_world, lo, hi);
    sc[j] = scalars[j] + lo;
    bs[j] = bases[j] + lo;
    ln[j] = hi - lo;
  }
  return msm_multi_begin(pk->ctx, sc.data(), bs.data(), ln.data(), count, pend);
}
int Commit::end(std::vector<G1Affine>& out) {
  cq_ctx* c = pk->ctx;
  std::vector<uint64_t> jac(count * 12);
  const bool trace_host = host_trace_enabled();
  const auto t0 = std::chrono::steady_clock::now();
  if (trace_host) hipStreamSynchronize(c->stream);
  const auto t1 = std::chrono::steady_clock::now();
  int rc = msm_multi_end(c, pend, jac.data());
  if (rc != CQ_OK) return rc;
  const auto t2 = std::chrono::steady_clock::now();
  struct Report {
    bool on; std::chrono::steady_clock::time_point a, b, c_;
    ~Report() {
      if (on) fprintf(stderr, "[cq host]   commit end: wait %.1f us, fold %.1f us, exchange + normalise %.1f us\n",
                      std::chrono::duration<double, std::micro>(b - a).count(), std::chrono::duration<double, std::micro>(c_ - b).count(),
                      std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - c_).count());
    }
  } report{trace_host, t0, t1, t2};
  std::vector<G1Jac> j(count);
  if (pk->sharded()) {
    // all-gather of count x 96 B per rank, then the local EC sum (not an RCCL reduction op)
    std::vector<uint64_t> all((size_t)pk->shard_world * count * 12);
    int arc = shard_allgather_host(pk, jac.data(), all.data(), count * 12 * sizeof(uint64_t));
    if (arc != CQ_OK) return arc;
    for (size_t i = 0; i < count; i++) {
      G1Jac acc = G1Jac::identity();
      for (uint32_t r = 0; r < pk->shard_world; r++) acc = jac_add(acc, jac_from_limbs(all.data() + ((size_t)r * count + i) * 12));
      j[i] = acc;
    }
  } else {
    for (size_t i = 0; i < count; i++) j[i] = jac_from_limbs(jac.data() + 12 * i);
  }
  batch_normalize(j, out);
  return CQ_OK;
}

int shard_any(const cq_pk* pk, bool flag, bool& out) {
  out = flag;
  if (!pk->sharded()) return CQ_OK;
  const uint64_t mine = flag ? 1 : 0;
  std::vector<uint64_t> all(pk->shard_world, 0);
  int arc = shard_allgather_host(pk, &mine, all.data(), sizeof(uint64_t));
  if (arc != CQ_OK) return arc;
  for (uint64_t v : all) out = out || v != 0;
  return CQ_OK;
}

int commit_batch_v(const cq_pk* pk, const std::vector<const Fr*>& scalars, const std::vector<const G1Affine*>& bases,
                   const std::vector<size_t>& lens, std::vector<G1Affine>& out) {
  Commit cm;
  int rc = cm.begin(pk, scalars, bases, lens);
  if (rc != CQ_OK) return rc;
  return cm.end(out);
}

int commit_batch(const cq_pk* pk, const std::vector<const Fr*>& scalars, const std::vector<const G1Affine*>& bases, size_t len,
                 std::vector<G1Affine>& out) {
  std::vector<size_t> lens(scalars.size(), len);
  return commit_batch_v(pk, scalars, bases, lens, out);
}

bool early_advice_polys(const cq_pk* pk) {
  return !pk->general() && pk->perm_sets() == 0 && pk->num_phases == 1 && pk->num_advice > 0 && !pk->lookups.empty();
}

void carve(const cq_pk* pk, Arena& ar, Buffers& b) {
  const size_t n = (size_t)1 << pk->k, ext = pk->domain->ext();
  const size_t L = pk->lookups.size(), A = pk->num_advice, I = pk->num_instance, S = pk->perm_sets();
  const size_t N = pk->table_cfg ? pk->table_cfg->N : 0;
  const bool general = pk->general();
  size_t wsum = 0;
  for (auto& lk : pk->lookups) wsum += lk.cols.size();
  const size_t npts = pk->opening_rotations().size();
  b.adv = ar.take(A * n);            // advice (lagrange -> coeff in place)
  // CQ-only single-phase circuits: the coefficient forms go to a buffer of their own, so that the transform can start
  // under the advice launch's tail while the Lagrange values are still needed (round 1 folds them into f)
  b.adv_coeff = ar.take(early_advice_polys(pk) ? A * n : 0);
  b.inst_lag = ar.take(I * n);
  b.inst_coeff = ar.take(I * n);
  b.f_lag = ar.take(L * n);
  b.f_coeff = ar.take(L * n);
  b.bpoly = ar.take(L * n);
  b.den = ar.take(L * N + 8);        // directly after bpoly: both are inverted by one batch inversion
  b.random_poly = ar.take(n);
  b.z = ar.take(S * n);              // permutation products (lagrange -> coeff in place)
  b.mv = ar.take(S * n);
  b.cosets = ar.take(2 * L * ext);   // b, f on the extended coset
  b.adv_cosets = ar.take(general ? A * ext : 0);
  b.inst_cosets = ar.take(general ? I * ext : 0);
  b.z_cosets = ar.take(S * ext);
  b.lk_inputs = ar.take(pk->lookup_exprs ? wsum * n : 0);  // evaluated input expressions of the static lookups
  // legacy lookups, per lookup: compressed input / table, permuted input / table, product (n each; the last three
  // become coefficients in place) and the five extended-coset vectors of its quotient terms
  b.plk = ar.take(pk->legacy.size() * 5 * n);
  b.plk_cosets = ar.take(pk->legacy.size() * 5 * ext);
  b.h_ext = ar.take(ext);
  b.h_coeff = ar.take(ext);          // n * (degree - 1) coefficients
  const bool shplonk = pk->opener == CQ_OPENER_SHPLONK;
  b.gwc_batch = ar.take(shplonk ? 0 : npts * n);
  b.gwc_wit = ar.take(shplonk ? 0 : npts * n);
  b.shplonk = ar.take(shplonk ? 5 * n + 64 * 8 : 0);  // h, two division buffers, h_x, l_x, low-degree remainders
  b.a_val = ar.take(L * N);
  b.m_fr = ar.take(L * N);
  b.a_scaled = ar.take(wsum * N);
  // (an even element count: the 64-byte points behind it stay 64-byte aligned)
  b.b_values = ar.take(pk->b_row_bases[0] ? (L * (N + 1) + 1) & ~(size_t)1 : 0);
  b.b_sums = (G1Affine*)ar.take(pk->b_row_bases[0] ? 2 * 2 * L * (N + 1) : 0);
  b.b_index = (uint32_t*)ar.take(pk->b_row_bases[0] ? (L * n + 7) / 8 : 0);  // L * n words of 4 bytes
  b.challenges = ar.take(pk->challenge_phase.size() + 8);
  b.tails = ar.take(A * (pk->bf + 1) + 8);
  b.gather = ar.take(GATHER_MAX);
  b.rng_dev = (uint64_t*)ar.take(2 * n);  // 64 B per element = 2 Fr
  b.m_counts = (uint32_t*)ar.take(L * N / 8 + 64);
  b.err_dev = b.m_counts ? b.m_counts + L * N : nullptr;
}

int lincomb_many(cq_ctx* c, const std::vector<Term>& terms, const Fr& sub_const, uint32_t n, Fr* out) {
  size_t done = 0;
  bool first = true;
  do {
    LincombArgs la;
    la.count = 0;
    la.sub_const = Fr::zero();
    if (!first) {
      la.p[0] = out;
      la.len[0] = n;
      la.coeff[0] = Fr::one();
      la.count = 1;
    }
    while (done < terms.size() && la.count < LINCOMB_MAX) {
      la.p[la.count] = terms[done].p;
      la.len[la.count] = terms[done].len;
      la.coeff[la.count] = terms[done].coeff;
      la.count++;
      done++;
    }
    if (done == terms.size()) la.sub_const = sub_const;
    int rc = poly_lincomb(c, la, n, out);
    if (rc != CQ_OK) return rc;
    first = false;
  } while (done < terms.size());
  return CQ_OK;
}

int eval_many(cq_ctx* c, const std::vector<const Fr*>& ps, const std::vector<uint32_t>& ls, const Fr& z, Fr* out) {
  for (size_t off = 0; off < ps.size(); off += EVAL_MAX_BATCH) {
    const uint32_t cnt = (uint32_t)std::min((size_t)EVAL_MAX_BATCH, ps.size() - off);
    int rc = poly_eval_batch(c, ps.data() + off, ls.data() + off, cnt, z, out + off);
    if (rc != CQ_OK) return rc;
  }
  return CQ_OK;
}

void RandomPolyDrawer::start(cq_ctx* c, Rng* rng, uint64_t* pin, uint64_t* dev, size_t words) {
  const size_t chunk = std::max<size_t>(words / 4, (size_t)1 << 18);  // each drawn by up to eight threads, uploaded while the next is drawn
  chunks_total = (uint32_t)((words + chunk - 1) / chunk);
  t_start = std::chrono::steady_clock::now();
  auto work = [=]() {
    hipError_t e = hipSetDevice(c->device);
    for (size_t off = 0; off < words && e == hipSuccess; off += chunk) {
      const size_t cnt = std::min(chunk, words - off);
      rng->fill(pin + off, cnt);
      e = hipMemcpyAsync(dev + off, pin + off, cnt * sizeof(uint64_t), hipMemcpyHostToDevice, c->copy_stream);
      chunks_done.fetch_add(1);
    }
    (void)rng->fr();  // random_blind
    if (e == hipSuccess) e = hipEventRecord(c->copy_done, c->copy_stream);
    err = e;
    done.store(true);
  };
  try {
    th = std::thread(work);
    running = true;
  } catch (...) {  // no thread to be had: draw here (nothing may unwind across the C ABI)
    work();
  }
}
int RandomPolyDrawer::join() {
  if (running) {
    th.join();
    running = false;
  }
  return err == hipSuccess ? 0 : -1;
}

}  // namespace prover
}  // namespace cq

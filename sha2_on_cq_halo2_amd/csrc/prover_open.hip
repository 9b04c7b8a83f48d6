// Evaluations and the multi-open argument: ProverGWC and ProverSHPLONK over a list of queries (shared with stage_multiopen,
// prover_stages.hip), and ProofRun's evaluate_and_write, open_gwc and open_shplonk.
#include "prover_run.hpp"

namespace cq {
namespace prover {

namespace {

// lagrange_interpolate (arithmetic.rs:425-478) of a commitment's evaluations over its set's points
std::vector<Fr> lagrange_interpolate(const std::vector<Fr>& pts, const std::vector<Fr>& evals) {
  const size_t m = pts.size();
  if (m == 1) return std::vector<Fr>{evals[0]};
  std::vector<Fr> fin(m, Fr::zero());
  for (size_t j = 0; j < m; j++) {
    std::vector<Fr> tmp{Fr::one()};
    for (size_t kk = 0; kk < m; kk++) {
      if (kk == j) continue;
      const Fr denom = (pts[j] - pts[kk]).inv();
      std::vector<Fr> nxt(tmp.size() + 1, Fr::zero());
      for (size_t i = 0; i <= tmp.size(); i++) {
        const Fr a_ = i < tmp.size() ? tmp[i] : Fr::zero();
        const Fr b_ = i > 0 ? tmp[i - 1] : Fr::zero();
        nxt[i] = a_ * (Fr::zero() - denom * pts[kk]) + b_ * denom;
      }
      tmp.swap(nxt);
    }
    for (size_t i = 0; i < m; i++) fin[i] = fin[i] + tmp[i] * evals[j];
  }
  return fin;
}
Fr eval_small(const std::vector<Fr>& poly, const Fr& at) {
  Fr acc = Fr::zero();
  for (size_t i = poly.size(); i-- > 0;) acc = acc * at + poly[i];
  return acc;
}

Fr h_value(const OpenJob& j) {  // h(x) = sum_i xn^i h_i(x) (vanishing/prover.rs:131-135)
  Fr h_eval = Fr::zero();
  for (size_t i = j.q_h->size(); i-- > 0;) h_eval = h_eval * j.xn + (*j.qs)[(*j.q_h)[i]].eval;
  return h_eval;
}

}  // namespace

// ---- multiopen, GWC (gwc/prover.rs:42-91): one witness polynomial per distinct point ---------------------
int open_gwc_queries(OpenJob& j) {
  const cq_pk* pk = j.pk;
  cq_ctx* c = pk->ctx;
  const size_t n = (size_t)1 << pk->k, pieces = j.q_h->size();
  const std::vector<Query>& qs = *j.qs;
  Fr v;
  CQ_TRY(j.tr.squeeze(v));
  const Fr h_eval = h_value(j);  // its value follows from the piece evaluations
  std::vector<const Fr*> sc;
  for (size_t g = 0; g < j.points->size(); g++) {
    std::vector<Term> terms;
    Fr pv = Fr::one(), eval_batch = Fr::zero(), xp = Fr::one();
    for (auto& q : qs) {
      if (q.pt != g) continue;
      if (q.h_piece >= 0) {  // the pieces of h share one power of v
        terms.push_back({q.p, q.len, pv * xp});
        xp = xp * j.xn;
        if ((size_t)q.h_piece + 1 < pieces) continue;
        eval_batch = eval_batch + h_eval * pv;
      } else {
        terms.push_back({q.p, q.len, pv});
        eval_batch = eval_batch + q.eval * pv;
      }
      pv = pv * v;
    }
    Fr* batch = j.gwc_batch + g * n;
    Fr* wit = j.gwc_wit + g * n;
    if (j.witness) {
      CQ_TRY(j.witness(g, terms, eval_batch, batch, wit));
    } else {
      CQ_TRY(lincomb_many(c, terms, eval_batch, (uint32_t)n, batch));  // poly_batch - eval_batch (gwc/prover.rs:62-78)
      CQ_TRY(poly_kate_division(c, batch, (uint32_t)n, (*j.points)[g], wit));  // :80
    }
    sc.push_back(wit);
  }
  std::vector<const G1Affine*> bs(sc.size(), pk->params->g);
  std::vector<G1Affine> o;
  CQ_TRY(commit_batch(pk, sc, bs, n - 1, o));  // :85
  for (auto& w : o) CQ_TRY(j.tr.write_point(w, "opening witness commitment is the identity"));
  return CQ_OK;
}

// ---- multiopen, SHPLONK (shplonk/prover.rs:120-286): two commitments whatever the number of points ---------
int open_shplonk_queries(OpenJob& j) {
  const cq_pk* pk = j.pk;
  cq_ctx* c = pk->ctx;
  const hipStream_t s = c->stream;
  const size_t n = (size_t)1 << pk->k, pieces = j.q_h->size();
  const std::vector<Query>& qs = *j.qs;
  const std::vector<Fr>& points = *j.points;
  Fr* sh_h = j.shplonk;           // h(X) = sum_i xn^i h_i as one polynomial (vanishing/prover.rs:131-135)
  Fr* sh_div[2] = {j.shplonk + n, j.shplonk + 2 * n};
  Fr* sh_hx = j.shplonk + 3 * n;
  Fr* sh_lx = j.shplonk + 4 * n;
  Fr* sh_rem = j.shplonk + 5 * n;  // per rotation set: sum_j y^j r_j (at most 8 coefficients)
  const Fr h_eval = h_value(j);
  if (pieces) {
    std::vector<Term> terms;
    Fr xp = Fr::one();
    for (size_t i = 0; i < pieces; i++) {
      const Query& q = qs[(*j.q_h)[i]];
      terms.push_back({q.p, q.len, xp});
      xp = xp * j.xn;
    }
    CQ_TRY(lincomb_many(c, terms, Fr::zero(), (uint32_t)n, sh_h));
  }
  Fr y_;
  CQ_TRY(j.tr.squeeze(y_));  // :136
  // construct_intermediate_sets (shplonk.rs:56-133): commitments by polynomial identity, grouped by point set
  struct Com { const Fr* p; uint32_t len; std::vector<uint32_t> pts; std::vector<Fr> evals; };
  std::vector<Com> coms;
  for (auto& q : qs) {
    const Fr* key = q.h_piece >= 0 ? sh_h : q.p;
    if (q.h_piece > 0) continue;
    const Fr ev = q.h_piece == 0 ? h_eval : q.eval;
    auto it = std::find_if(coms.begin(), coms.end(), [&](const Com& cm) { return cm.p == key; });
    if (it == coms.end()) {
      coms.push_back({key, q.h_piece == 0 ? (uint32_t)n : q.len, {q.pt}, {ev}});
    } else if (std::find(it->pts.begin(), it->pts.end(), q.pt) == it->pts.end()) {
      it->pts.push_back(q.pt);
      it->evals.push_back(ev);
    }
  }
  struct RotSet { std::vector<uint32_t> pts; std::vector<size_t> members; };
  std::vector<RotSet> sets;
  auto same_set = [](const std::vector<uint32_t>& a, const std::vector<uint32_t>& b) {
    return a.size() == b.size() && std::all_of(a.begin(), a.end(), [&](uint32_t r) { return std::find(b.begin(), b.end(), r) != b.end(); });
  };
  for (size_t ci = 0; ci < coms.size(); ci++) {
    auto it = std::find_if(sets.begin(), sets.end(), [&](const RotSet& rs) { return same_set(rs.pts, coms[ci].pts); });
    if (it == sets.end()) sets.push_back({coms[ci].pts, {ci}});
    else it->members.push_back(ci);
  }
  if (sets.size() > 64) return c->fail(CQ_ERR_ARG, "too many rotation sets");
  Fr v_;
  CQ_TRY(j.tr.squeeze(v_));  // :196
  // per set: low-degree equivalents r_j and the y-combined remainder (CommitmentExtension, :36-76)
  std::vector<std::vector<Fr>> set_points(sets.size());
  std::vector<std::vector<std::vector<Fr>>> low(sets.size());
  std::vector<Fr> rem_host(sets.size() * 8, Fr::zero());
  for (size_t si = 0; si < sets.size(); si++) {
    for (uint32_t r : sets[si].pts) set_points[si].push_back(points[r]);
    if (set_points[si].size() > 8) return c->fail(CQ_ERR_ARG, "rotation set too large");
    Fr py = Fr::one();
    for (size_t ci : sets[si].members) {
      // the commitment's evaluations, aligned with the set's point order
      std::vector<Fr> evals;
      for (uint32_t r : sets[si].pts) {
        const size_t pos = std::find(coms[ci].pts.begin(), coms[ci].pts.end(), r) - coms[ci].pts.begin();
        evals.push_back(coms[ci].evals[pos]);
      }
      low[si].push_back(lagrange_interpolate(set_points[si], evals));
      for (size_t i = 0; i < low[si].back().size(); i++) rem_host[si * 8 + i] = rem_host[si * 8 + i] + py * low[si].back()[i];
      py = py * y_;
    }
  }
  CQ_HIP(c, hipMemcpyAsync(sh_rem, rem_host.data(), rem_host.size() * sizeof(Fr), hipMemcpyHostToDevice, s));
  // h_x = sum_i v^i * (sum_j y^j (p_j - r_j)) / prod_{pt in set_i} (X - pt)   (quotient_contribution, :138-168)
  Fr pv = Fr::one();
  for (size_t si = 0; si < sets.size(); si++) {
    std::vector<Term> terms;
    Fr py = Fr::one();
    for (size_t ci : sets[si].members) {
      terms.push_back({coms[ci].p, coms[ci].len, py});
      py = py * y_;
    }
    terms.push_back({sh_rem + si * 8, (uint32_t)set_points[si].size(), Fr::zero() - Fr::one()});
    CQ_TRY(lincomb_many(c, terms, Fr::zero(), (uint32_t)n, sh_div[0]));
    uint32_t len = (uint32_t)n;
    int cur = 0;
    for (const Fr& pt : set_points[si]) {  // div_by_vanishing (:28-34)
      CQ_TRY(poly_kate_division(c, sh_div[cur], len, pt, sh_div[cur ^ 1]));
      cur ^= 1;
      len--;
    }
    std::vector<Term> acc;
    if (si) acc.push_back({sh_hx, (uint32_t)n, Fr::one()});
    acc.push_back({sh_div[cur], len, pv});
    CQ_TRY(lincomb_many(c, acc, Fr::zero(), (uint32_t)n, sh_hx));
    pv = pv * v_;
  }
  {
    std::vector<const Fr*> sc{sh_hx};
    std::vector<const G1Affine*> bs{pk->params->g};
    std::vector<G1Affine> o;
    CQ_TRY(commit_batch(pk, sc, bs, n, o));  // :204
    CQ_TRY(j.tr.write_point(o[0], "shplonk quotient commitment is the identity"));
  }
  Fr u_;
  CQ_TRY(j.tr.squeeze(u_));  // :206
  // l_x = sum_i v^i z_i sum_j y^j (p_j - r_j(u)) - Z_T(u) h_x, then / (X - u) and / z_0   (:208-283); the
  // scaling by 1/z_0 is folded into the coefficients (the division is linear)
  auto vanish = [&](const std::vector<Fr>& roots) {
    Fr acc = Fr::one();
    for (auto& r : roots) acc = (u_ - r) * acc;
    return acc;
  };
  std::vector<Fr> z_diff(sets.size());
  for (size_t si = 0; si < sets.size(); si++) {
    std::vector<Fr> diffs;
    for (uint32_t pi = 0; pi < points.size(); pi++)  // super_point_set: every distinct point
      if (std::find(sets[si].pts.begin(), sets[si].pts.end(), pi) == sets[si].pts.end()) diffs.push_back(points[pi]);
    z_diff[si] = vanish(diffs);
  }
  const Fr z0_inv = z_diff[0].inv();
  const Fr zt_eval = vanish(points);
  std::vector<Term> terms;
  Fr sub = Fr::zero();
  pv = Fr::one();
  for (size_t si = 0; si < sets.size(); si++) {
    const Fr scale = pv * z_diff[si] * z0_inv;
    Fr py = Fr::one();
    for (size_t m = 0; m < sets[si].members.size(); m++) {
      const Com& cm = coms[sets[si].members[m]];
      terms.push_back({cm.p, cm.len, scale * py});
      sub = sub + scale * py * eval_small(low[si][m], u_);
      py = py * y_;
    }
    pv = pv * v_;
  }
  terms.push_back({sh_hx, (uint32_t)n, Fr::zero() - zt_eval * z0_inv});
  CQ_TRY(lincomb_many(c, terms, sub, (uint32_t)n, sh_lx));
  CQ_TRY(poly_kate_division(c, sh_lx, (uint32_t)n, u_, sh_div[0]));  // :257
  std::vector<const Fr*> sc{sh_div[0]};
  std::vector<const G1Affine*> bs{pk->params->g};
  std::vector<G1Affine> o;
  CQ_TRY(commit_batch(pk, sc, bs, n - 1, o));  // :270
  return j.tr.write_point(o[0], "shplonk opening commitment is the identity");
}

// ---- evaluations (prover.rs:654-719) and opening queries (:721-773) ------------------------------------
int ProofRun::evaluate_and_write() {
  const int32_t rot_last = -(int32_t)(bf + 1);
  std::vector<size_t> q_advice, q_fixed, q_sigma, q_z, q_z_next, q_z_last(S, (size_t)-1), q_b0, q_f;
  for (auto& q : pk->advice_queries) q_advice.push_back(add_query(adv_poly + (size_t)q.first * n, n, q.second));
  for (size_t st = 0; st < S; st++) {  // permutation::Evaluated::open (permutation/prover.rs:294-344)
    q_z.push_back(add_query(B.z + st * n, n, 0));
    q_z_next.push_back(add_query(B.z + st * n, n, 1));
  }
  for (size_t st = S > 0 ? S - 1 : 0; st-- > 0;) q_z_last[st] = add_query(B.z + st * n, n, rot_last);
  std::vector<std::array<size_t, 5>> q_plk(PL);  // lookup::Evaluated::open (lookup/prover.rs:343-392): z, a', s' @ x, a' @ x/w, z @ wx
  for (size_t l = 0; l < PL; l++)
    q_plk[l] = {add_query(plk_buf(l, 4), n, 0), add_query(plk_buf(l, 2), n, 0), add_query(plk_buf(l, 3), n, 0),
                add_query(plk_buf(l, 2), n, -1), add_query(plk_buf(l, 4), n, 1)};
  for (size_t l = 0; l < L; l++) {  // static_lookup::Evaluated::open
    q_b0.push_back(add_query(B.bpoly + l * n + 1, n - 1, 0));  // b0 = (b - b(0))/X
    q_f.push_back(add_query(B.f_coeff + l * n, n, 0));
  }
  for (auto& q : pk->fixed_queries) q_fixed.push_back(add_query(pk->fixed_polys + (size_t)q.first * n, n, q.second));
  for (size_t ci = 0; ci < PC; ci++) q_sigma.push_back(add_query(pk->perm_polys + ci * n, n, 0));  // ProvingKey::open (:215-225)
  for (size_t i = 0; i < pieces; i++) {
    q_h.push_back(add_query(B.h_coeff + i * n, n, 0));
    qs.back().h_piece = (int)i;
  }
  const size_t q_random = add_query(B.random_poly, n, 0);
  // distinct points in first-seen order (gwc.rs:36-61)
  for (auto& q : qs) {
    if (std::find(rots.begin(), rots.end(), q.rot) == rots.end()) rots.push_back(q.rot);
    q.pt = (uint32_t)(std::find(rots.begin(), rots.end(), q.rot) - rots.begin());
  }
  for (int32_t rot : rots) points.push_back(point_of(rot));
  if (resident) {
    CQ_TRY(resident_evaluate(q_advice, q_b0, q_f));
  } else {
    for (int32_t rot : rots) {
      std::vector<const Fr*> ps;
      std::vector<uint32_t> ls;
      std::vector<size_t> idx;
      for (size_t i = 0; i < qs.size(); i++)
        if (qs[i].rot == rot) {
          ps.push_back(qs[i].p);
          ls.push_back(qs[i].len);
          idx.push_back(i);
        }
      std::vector<Fr> ev(ps.size());
      CQ_TRY(eval_many(c, ps, ls, point_of(rot), ev.data()));
      for (size_t j = 0; j < idx.size(); j++) qs[idx[j]].eval = ev[j];
    }
  }
  for (size_t i : q_advice) tr.write_scalar(qs[i].eval);  // :654-672
  for (size_t i : q_fixed) tr.write_scalar(qs[i].eval);   // :674-687
  tr.write_scalar(qs[q_random].eval);                     // vanishing/prover.rs:145-146
  for (size_t i : q_sigma) tr.write_scalar(qs[i].eval);   // permutation/prover.rs:227-239
  for (size_t st = 0; st < S; st++) {                     // :243-290
    tr.write_scalar(qs[q_z[st]].eval);
    tr.write_scalar(qs[q_z_next[st]].eval);
    if (st + 1 < S) tr.write_scalar(qs[q_z_last[st]].eval);
  }
  for (size_t l = 0; l < PL; l++)  // lookup::Committed::evaluate (lookup/prover.rs:303-340): z, z(wx), a', a'(x/w), s'
    for (size_t which : {(size_t)0, (size_t)4, (size_t)1, (size_t)3, (size_t)2}) tr.write_scalar(qs[q_plk[l][which]].eval);
  for (size_t l = 0; l < L; l++) {  // static_lookup/prover.rs:360-370
    tr.write_scalar(qs[q_b0[l]].eval);
    tr.write_scalar(qs[q_f[l]].eval);
    tr.write_scalar(a_at_zero[l]);
  }
  return CQ_OK;
}

// ---- multiopen over the proof's queries: ProverGWC (gwc/prover.rs:42-91) or ProverSHPLONK (shplonk/prover.rs:120-286)
OpenJob ProofRun::open_job() {
  OpenJob j;
  j.pk = pk;
  j.qs = &qs;
  j.points = &points;
  j.q_h = &q_h;
  j.xn = xn;
  j.gwc_batch = B.gwc_batch;
  j.gwc_wit = B.gwc_wit;
  j.shplonk = B.shplonk;
  j.tr.squeeze = [this](Fr& out) {
    out = tr.squeeze();
    return (int)CQ_OK;
  };
  j.tr.write_point = [this](const G1Affine& p, const char* what) { return tr.write_point(p) ? (int)CQ_OK : c->fail(CQ_ERR_TRANSCRIPT, what); };
  return j;
}
int ProofRun::open_shplonk() {
  OpenJob j = open_job();
  return open_shplonk_queries(j);
}
int ProofRun::open_gwc() {
  OpenJob j = open_job();
  if (resident)
    j.witness = [this](size_t g, const std::vector<Term>& terms, const Fr& eval_batch, Fr* batch, Fr* wit) {
      return resident_witness(g, terms, eval_batch, batch, wit);
    };
  return open_gwc_queries(j);
}

}  // namespace prover
}  // namespace cq

// G1 MSM engine, above the launches: the window width of the tables, the planner that cuts a list of MSMs into launches and
// folds their results (msm_multi_begin / msm_multi_end, cq_msm_multi{,_v}), and the registry of the window tables.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "ctx.hpp"
#include "msm.hpp"

using namespace cq;

uint32_t msm_table_window_bits(size_t n) {
  if (const char* e = getenv("CQ_TABLE_C")) {
    const long v = atol(e);
    if (v >= (long)MSM_TABLE_C_MIN && v <= (long)MSM_TABLE_C_MAX) return (uint32_t)v;
  }
  // Measured on MI355X, whole proofs of the SHA-shaped circuit (tools/table_c_sweep.sh; ms at c = 15 / 16 / 17 / 18 / 20):
  //   k = 18:  8.2 /  8.6 /  9.4 /  14.0 / 16.3      k = 20: 26.5 / 26.0 / 25.4 / 32.4 / 33.9      k = 22: 97.2 / 94.0 / 92.3 / 115 / 99
  // 17 bits: 15 instead of 17 additions per scalar, 2^16 buckets per MSM that the two-pass sort still reaches with a byte
  // per entry; beyond, the third sort pass and the 2^17..2^19-bucket reductions cost more than the additions saved.
  return n >= ((size_t)1 << 20) ? 17u : MSM_TABLE_C;
}

static uint32_t pick_c(cq_ctx* c, uint32_t n) {
  if (c->msm_c) return c->msm_c;
  return msm_window_bits(n);
}

// Runs `count` MSMs (each with its own base array and length); results to host Jacobians.
// Base arrays registered with cq_msm_precompute use their per-window tables (one bucket set per MSM,
// no window folding on the host) and may share a launch whatever their lengths; plain MSMs are
// grouped by equal length, and a group of at most MSM_SHORT_MAX terms takes the one-kernel short path (msm_short_run)
// unless the caller fixed the window width of the generic pipeline (cq_msm_set_window).
int msm_multi_begin(cq_ctx* c, const Fr* const* scalars, const G1Affine* const* bases, const size_t* lens, size_t count,
                    MsmPending& pend) {
  pend.launches.clear();
  pend.count = count;
  for (size_t j = 0; j < count; j++)
    if (lens[j] > 0x7fffffffull) return c->fail(CQ_ERR_ARG, "msm: len too large");
  // Tables of one width share a launch: where an array has several (a small table SRS next to SRS arrays of different
  // sizes), take the width of the longest MSM's table.
  uint32_t want_c = 0;
  {
    size_t longest = 0;
    for (size_t j = 0; j < count; j++)
      if (lens[j] > longest)
        if (const cq_ctx::MsmTable* t = c->find_msm_table(bases[j], lens[j])) { longest = lens[j]; want_c = t->c; }
  }
  // first pass: plan the launches and the result slots
  size_t done = 0, slots = 0;
  while (done < count) {
    MsmPending::Launch ln;
    ln.first = done;
    if (lens[done] == 0) {
      ln.batch = 1;
      ln.empty = true;
      pend.launches.push_back(ln);
      done++;
      continue;
    }
    const cq_ctx::MsmTable* t0 = c->find_msm_table(bases[done], lens[done], nullptr, want_c);
    const bool pre = t0 != nullptr;
    uint32_t nmax = (uint32_t)lens[done];
    uint32_t batch = 1;
    while (done + batch < count && batch < MSM_MAX_BATCH) {
      const size_t l = lens[done + batch];
      if (l == 0) break;
      const cq_ctx::MsmTable* t = c->find_msm_table(bases[done + batch], l, nullptr, want_c);
      if ((t != nullptr) != pre) break;
      if (pre && t->c != t0->c) break;
      if (!pre && l != lens[done]) break;
      nmax = std::max(nmax, (uint32_t)l);
      batch++;
    }
    ln.short_path = !pre && !c->msm_c && nmax <= MSM_SHORT_MAX;
    const uint32_t cb = pre ? t0->c : ln.short_path ? MSM_SHORT_C : pick_c(c, nmax);
    // keep the workspace below ~32 GiB (of 288): the layout of every candidate batch size once, the one that fits is the launch's
    ln.L.emplace(nmax, cb, batch, pre);
    while (batch > 1 && ln.L->total > ((size_t)32 << 30)) {
      batch = (batch + 1) / 2;
      ln.L.emplace(nmax, cb, batch, pre);
    }
    ln.batch = batch;
    ln.slot = slots;
    slots += (size_t)MSM_SET_POINTS * batch * ln.L->Wb;  // bit-plane sums of every bucket set
    pend.launches.push_back(ln);
    done += batch;
  }
  void *wsums = nullptr, *host = nullptr;
  int rc;
  if (slots) {
    if ((rc = c->ensure_scratch(Scratch::MsmSums, slots * sizeof(G1Jac), &wsums)) != CQ_OK) return rc;
    if ((rc = c->ensure_pinned_msm(slots * sizeof(G1Jac), &host)) != CQ_OK) return rc;
  }
  pend.host = host;
  pend.slots = slots;
  for (auto& ln : pend.launches) {
    if (ln.empty) continue;
    const MsmLayout& L = *ln.L;
    if (ln.short_path) {  // same result layout as a plain launch of 8-bit windows: 32 one-row bucket sets per MSM
      void* ws;
      if ((rc = c->ensure_scratch(Scratch::MsmWork, msm_short_workspace(L.n, ln.batch), &ws)) != CQ_OK) return rc;
      if (msm_short_run(c, scalars + ln.first, bases + ln.first, L.n, ln.batch, ws, (G1Jac*)wsums + ln.slot) != 0)
        return c->fail(CQ_ERR_HIP, "msm launch failed");
      continue;
    }
    std::vector<const G1Affine*> bp(ln.batch);
    std::vector<size_t> strides(ln.batch, 0);
    for (uint32_t j = 0; j < ln.batch; j++) {
      size_t toff = 0;
      const cq_ctx::MsmTable* t = L.pre ? c->find_msm_table(bases[ln.first + j], lens[ln.first + j], &toff, L.c) : nullptr;
      bp[j] = L.pre ? (const G1Affine*)t->table + toff : bases[ln.first + j];
      strides[j] = L.pre ? t->n : 0;
    }
    void* ws;
    if ((rc = c->ensure_scratch(Scratch::MsmWork, L.total, &ws)) != CQ_OK) return rc;
    const MsmLaunch run{false, (const void* const*)(scalars + ln.first), bp.data(),
                        lens + ln.first, strides.data(), (G1Jac*)wsums + ln.slot, nullptr, 0};
    if (msm_run(c, run, L, ws) != 0) return c->fail(CQ_ERR_HIP, "msm launch failed");
  }
  if (slots)
    CQ_HIP(c, hipMemcpyAsync(host, wsums, slots * sizeof(G1Jac), hipMemcpyDeviceToHost, c->stream));
  return CQ_OK;
}

int msm_multi_end(cq_ctx* c, MsmPending& pend, uint64_t* out_jac) {
  if (int wrc = c->wait(c->stream, "msm: waiting for the launch")) return wrc;
  // the host's share of the reduction (msm_set_value: ~33 group operations per bucket set), spread over the context's
  // worker threads when a launch has many sets
  struct Item { const MsmPending::Launch* ln; uint32_t j; };
  std::vector<Item> items;
  size_t sets = 0;
  for (auto& ln : pend.launches)
    for (uint32_t j = 0; j < ln.batch; j++) {
      items.push_back({&ln, j});
      if (!ln.empty) sets += ln.L->Wb;
    }
  const G1Jac* host = (const G1Jac*)pend.host;
  auto fold = [&](size_t i) {
    const MsmPending::Launch& ln = *items[i].ln;
    const uint32_t j = items[i].j;
    uint64_t* o = out_jac + (ln.first + j) * 12;
    if (ln.empty) {
      memset(o, 0, 12 * sizeof(uint64_t));
      return;
    }
    const G1Jac* res = host + ln.slot;
    const MsmLayout& L = *ln.L;
    G1Jac r = L.pre ? msm_fold_sets(res + (size_t)MSM_SET_POINTS * j * L.Wb, L.Wb, L.M, L.cols)
                    : msm_fold_windows(res + (size_t)MSM_SET_POINTS * j * L.W, L.W, L.c, L.cols);
    r.x.to_limbs64(o);
    r.y.to_limbs64(o + 4);
    r.z.to_limbs64(o + 8);
  };
  if (sets > 6) {
    c->pool().parallel_for(items.size(), fold);
  } else {
    for (size_t i = 0; i < items.size(); i++) fold(i);
  }
  return CQ_OK;
}

int cq_msm_multi_v(cq_ctx* c, const Fr* const* scalars, const G1Affine* const* bases, const size_t* lens, size_t count,
                   uint64_t* out_jac) {
  MsmPending pend;
  int rc = msm_multi_begin(c, scalars, bases, lens, count, pend);
  if (rc != CQ_OK) return rc;
  return msm_multi_end(c, pend, out_jac);
}

int cq_msm_multi(cq_ctx* c, const Fr* const* scalars, const G1Affine* const* bases, size_t len, size_t count,
                 uint64_t* out_jac) {
  std::vector<size_t> lens(count, len);
  return cq_msm_multi_v(c, scalars, bases, lens.data(), count, out_jac);
}

void msm_unregister_tables(cq_ctx* c, const void* bases) {
  for (size_t i = 0; i < c->msm_tables.size();) {
    if (c->msm_tables[i].bases == bases) {
      hipFree(c->msm_tables[i].table);
      c->msm_tables.erase(c->msm_tables.begin() + i);
    } else {
      i++;
    }
  }
}

void msm_release_table(cq_ctx* c, const void* bases, size_t n, uint32_t c_bits) {
  for (size_t i = 0; i < c->msm_tables.size(); i++) {
    cq_ctx::MsmTable& t = c->msm_tables[i];
    if (t.bases != bases || t.n != n || t.c != c_bits) continue;
    if (--t.refs == 0) {
      hipFree(t.table);
      c->msm_tables.erase(c->msm_tables.begin() + i);
    }
    return;
  }
}

// Builds and registers per-window tables T[w][i] = 2^(c*w) * bases[i] for a device-resident base array.
// Memory: ceil(255/c) x n x 64 B (17 x the SRS for n >= 2^15) -- sized for 288 GB of HBM.
int msm_register_tables(cq_ctx* c, const G1Affine* bases, size_t n, uint32_t want_c, bool* held) {
  if (held) *held = false;
  if (!bases || n == 0 || n > (1u << 26)) return CQ_OK;  // nothing to do / unsupported: plain mode
  // The width comes from the array's own length (15 bits up to 2^19 points, 17 from 2^20 on) unless the caller of the
  // library (cq_msm_set_table_window) or of this function (a proving key bringing its small arrays to the width of its
  // SRS, so that its MSMs share launches) says otherwise -- never from what happened to be registered first.
  const uint32_t cb = want_c ? want_c : (c->msm_table_c ? c->msm_table_c : msm_table_window_bits(n));
  for (auto& t : c->msm_tables)
    if (t.bases == bases && t.n == n && t.c == cb) {  // the very entry: one more holder
      t.refs++;
      if (held) *held = true;
      return CQ_OK;
    }
  {
    size_t off = 0;
    const cq_ctx::MsmTable* t = c->find_msm_table(bases, n, &off, cb);
    if (t && (t->c == cb || !want_c)) return CQ_OK;  // served by a registered (larger) array's table
  }
  const uint32_t W = (255 + cb - 1) / cb;
  void* table = nullptr;
  if (hipMalloc(&table, (size_t)W * n * sizeof(G1Affine)) != hipSuccess) {
    (void)hipGetLastError();
    return CQ_OK;  // not enough memory: stay in plain mode
  }
  if (msm_precompute_tables(c, bases, (uint32_t)n, cb, (G1Affine*)table) != 0) {
    hipFree(table);
    return c->fail(CQ_ERR_HIP, "msm precompute failed");
  }
  c->msm_tables.push_back({bases, n, cb, table, 1});
  if (held) *held = true;
  return CQ_OK;
}

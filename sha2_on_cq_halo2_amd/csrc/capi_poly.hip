// C ABI: EvaluationDomain transforms, eval_polynomial, kate_division, batch inversion (plain and of Assigned columns).
#include <cstring>
#include <string>
#include <vector>
#include "assigned_host.hpp"
#include "ctx.hpp"
#include "poly.hpp"

using namespace cq;

namespace {
struct HostStage {
  cq_ctx* c;
  void* din = nullptr;
  void* dout = nullptr;
  int rc = CQ_OK;
  HostStage(cq_ctx* c_, size_t in_bytes, size_t out_bytes) : c(c_) {
    if ((rc = c->ensure_scratch(Scratch::EntryA, in_bytes ? in_bytes : 32, &din)) != CQ_OK) return;
    rc = c->ensure_scratch(Scratch::EntryB, out_bytes ? out_bytes : 32, &dout);
  }
};

// the shape checks the two batch_invert_assigned entry points share; off[c] = entries before column c
int assigned_offsets(cq_ctx* c, const cq_assigned_column* cols, size_t ncols, size_t n, std::vector<uint32_t>& off) {
  if (n > 0x7fffffffull) return c->fail(CQ_ERR_ARG, "batch_invert_assigned: n too large");
  off.assign(ncols + 1, 0);
  for (size_t a = 0; a < ncols; a++) {
    const cq_assigned_column& col = cols[a];
    if ((n && !col.num) || (col.den_count && (!col.den_rows || !col.den)))
      return c->fail(CQ_ERR_ARG, "batch_invert_assigned: column " + std::to_string(a) + ": null array");
    if (col.den_count > n)  // rows ascend strictly below n: more than n of them cannot be a good list
      return c->fail(CQ_ERR_ARG, "batch_invert_assigned: column " + std::to_string(a) + ", entry " + std::to_string(n) +
                                     ": more entries than rows");
    if ((uint64_t)off[a] + col.den_count > 0x7fffffffull) return c->fail(CQ_ERR_ARG, "batch_invert_assigned: too many rational cells");
    off[a + 1] = off[a] + (uint32_t)col.den_count;
  }
  return CQ_OK;
}
inline size_t round32(size_t b) { return (b + 31) & ~(size_t)31; }
}  // namespace

extern "C" {

int cq_domain_create(cq_ctx* c, uint32_t j, uint32_t k, cq_domain** out) {
  if (!c || !out || j < 1) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  return domain_create(c, j, k, out);
}
void cq_domain_destroy(cq_domain* d) { domain_destroy(d); }
uint32_t cq_domain_k(const cq_domain* d) { return d ? d->k : 0; }
uint32_t cq_domain_extended_k(const cq_domain* d) { return d ? d->extended_k : 0; }

int cq_domain_constants(const cq_domain* d, uint64_t omega[4], uint64_t omega_inv[4], uint64_t extended_omega[4],
                        uint64_t ifft_divisor[4]) {
  if (!d) return CQ_ERR_ARG;
  if (omega) d->omega.to_limbs64(omega);
  if (omega_inv) d->omega_inv.to_limbs64(omega_inv);
  if (extended_omega) d->extended_omega.to_limbs64(extended_omega);
  if (ifft_divisor) d->ifft_divisor.to_limbs64(ifft_divisor);
  return CQ_OK;
}

int cq_lagrange_to_coeff_dev(cq_domain* d, const uint64_t* in_dev, uint64_t* out_dev, uint32_t batch) {
  if (!d || !in_dev || !out_dev || !batch) return CQ_ERR_ARG;
  CQ_HIP(d->ctx, hipSetDevice(d->ctx->device));
  return domain_lagrange_to_coeff(d, (const Fr*)in_dev, (Fr*)out_dev, batch, d->n(), d->n());
}
int cq_coeff_to_extended_dev(cq_domain* d, const uint64_t* in_dev, uint64_t* out_dev, uint32_t batch) {
  if (!d || !in_dev || !out_dev || !batch) return CQ_ERR_ARG;
  if ((const void*)in_dev == (const void*)out_dev) return d->ctx->fail(CQ_ERR_ARG, "coeff_to_extended: in == out");
  CQ_HIP(d->ctx, hipSetDevice(d->ctx->device));
  return domain_coeff_to_extended(d, (const Fr*)in_dev, (Fr*)out_dev, batch, d->n(), d->ext());
}
int cq_extended_to_coeff_dev(cq_domain* d, const uint64_t* in_dev, uint64_t* out_dev) {
  if (!d || !in_dev || !out_dev) return CQ_ERR_ARG;
  CQ_HIP(d->ctx, hipSetDevice(d->ctx->device));
  return domain_extended_to_coeff(d, (const Fr*)in_dev, (Fr*)out_dev);
}

int cq_lagrange_to_coeff(cq_domain* d, uint64_t* a) {
  if (!d || !a) return CQ_ERR_ARG;
  cq_ctx* c = d->ctx;
  CQ_HIP(c, hipSetDevice(c->device));
  const size_t bytes = d->n() * sizeof(Fr);
  HostStage st(c, bytes, bytes);
  if (st.rc != CQ_OK) return st.rc;
  CQ_HIP(c, hipMemcpyAsync(st.din, a, bytes, hipMemcpyHostToDevice, c->stream));
  int rc = domain_lagrange_to_coeff(d, (const Fr*)st.din, (Fr*)st.dout, 1, d->n(), d->n());
  if (rc != CQ_OK) return rc;
  CQ_HIP(c, hipMemcpyAsync(a, st.dout, bytes, hipMemcpyDeviceToHost, c->stream));
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  return CQ_OK;
}
int cq_coeff_to_extended(cq_domain* d, const uint64_t* a, uint64_t* out) {
  if (!d || !a || !out) return CQ_ERR_ARG;
  cq_ctx* c = d->ctx;
  CQ_HIP(c, hipSetDevice(c->device));
  HostStage st(c, d->n() * sizeof(Fr), d->ext() * sizeof(Fr));
  if (st.rc != CQ_OK) return st.rc;
  CQ_HIP(c, hipMemcpyAsync(st.din, a, d->n() * sizeof(Fr), hipMemcpyHostToDevice, c->stream));
  int rc = domain_coeff_to_extended(d, (const Fr*)st.din, (Fr*)st.dout, 1, d->n(), d->ext());
  if (rc != CQ_OK) return rc;
  CQ_HIP(c, hipMemcpyAsync(out, st.dout, d->ext() * sizeof(Fr), hipMemcpyDeviceToHost, c->stream));
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  return CQ_OK;
}
int cq_extended_to_coeff(cq_domain* d, const uint64_t* a, uint64_t* out) {
  if (!d || !a || !out) return CQ_ERR_ARG;
  cq_ctx* c = d->ctx;
  CQ_HIP(c, hipSetDevice(c->device));
  const size_t out_bytes = d->n() * d->quotient_poly_degree * sizeof(Fr);
  HostStage st(c, d->ext() * sizeof(Fr), out_bytes);
  if (st.rc != CQ_OK) return st.rc;
  CQ_HIP(c, hipMemcpyAsync(st.din, a, d->ext() * sizeof(Fr), hipMemcpyHostToDevice, c->stream));
  int rc = domain_extended_to_coeff(d, (const Fr*)st.din, (Fr*)st.dout);
  if (rc != CQ_OK) return rc;
  if (out_bytes) CQ_HIP(c, hipMemcpyAsync(out, st.dout, out_bytes, hipMemcpyDeviceToHost, c->stream));
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  return CQ_OK;
}

int cq_eval_polynomial_dev(cq_ctx* c, const uint64_t* poly_dev, size_t n, const uint64_t point[4], uint64_t out[4]) {
  if (!c || !point || !out || (n && !poly_dev) || n > 0x7fffffffull) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  Fr r;
  int rc = poly_eval(c, (const Fr*)poly_dev, (uint32_t)n, Fr::from_limbs64(point), &r);
  if (rc != CQ_OK) return rc;
  r.to_limbs64(out);
  return CQ_OK;
}
int cq_eval_polynomial(cq_ctx* c, const uint64_t* poly, size_t n, const uint64_t point[4], uint64_t out[4]) {
  if (!c || !point || !out || (n && !poly) || n > 0x7fffffffull) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  HostStage st(c, n * sizeof(Fr), 32);
  if (st.rc != CQ_OK) return st.rc;
  if (n) CQ_HIP(c, hipMemcpyAsync(st.din, poly, n * sizeof(Fr), hipMemcpyHostToDevice, c->stream));
  return cq_eval_polynomial_dev(c, (const uint64_t*)st.din, n, point, out);
}

int cq_kate_division_dev(cq_ctx* c, const uint64_t* a_dev, size_t n, const uint64_t b[4], uint64_t* q_dev) {
  if (!c || !a_dev || !b || n == 0 || (n > 1 && !q_dev) || n > 0x7fffffffull) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  return poly_kate_division(c, (const Fr*)a_dev, (uint32_t)n, Fr::from_limbs64(b), (Fr*)q_dev);
}
int cq_kate_division(cq_ctx* c, const uint64_t* a, size_t n, const uint64_t b[4], uint64_t* q) {
  if (!c || !a || !b || n == 0 || (n > 1 && !q) || n > 0x7fffffffull) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  HostStage st(c, n * sizeof(Fr), n * sizeof(Fr));
  if (st.rc != CQ_OK) return st.rc;
  CQ_HIP(c, hipMemcpyAsync(st.din, a, n * sizeof(Fr), hipMemcpyHostToDevice, c->stream));
  int rc = poly_kate_division(c, (const Fr*)st.din, (uint32_t)n, Fr::from_limbs64(b), (Fr*)st.dout);
  if (rc != CQ_OK) return rc;
  if (n > 1) CQ_HIP(c, hipMemcpyAsync(q, st.dout, (n - 1) * sizeof(Fr), hipMemcpyDeviceToHost, c->stream));
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  return CQ_OK;
}

int cq_batch_invert_dev(cq_ctx* c, uint64_t* a_dev, size_t n) {
  if (!c || (n && !a_dev) || n > 0x7fffffffull) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  return poly_batch_invert(c, (Fr*)a_dev, (uint32_t)n);
}
int cq_batch_invert(cq_ctx* c, uint64_t* a, size_t n) {
  if (!c || (n && !a) || n > 0x7fffffffull) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  if (!n) return CQ_OK;
  HostStage st(c, n * sizeof(Fr), 32);
  if (st.rc != CQ_OK) return st.rc;
  CQ_HIP(c, hipMemcpyAsync(st.din, a, n * sizeof(Fr), hipMemcpyHostToDevice, c->stream));
  int rc = poly_batch_invert(c, (Fr*)st.din, (uint32_t)n);
  if (rc != CQ_OK) return rc;
  CQ_HIP(c, hipMemcpyAsync(a, st.din, n * sizeof(Fr), hipMemcpyDeviceToHost, c->stream));
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  return CQ_OK;
}


// batch_invert_assigned(_ref) (poly.rs:174-241) on device columns.  The columns' sparse lists are gathered behind one
// another in the entry scratch, checked there (a verdict cell, as the Processed readers use), and the resolve launches
// write nothing when the check objects.
int cq_batch_invert_assigned_dev(cq_ctx* c, const cq_assigned_column* cols, size_t ncols, size_t n, uint64_t* const* out_dev) {
  if (!c || (ncols && (!cols || !out_dev))) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  std::vector<uint32_t> off;
  int rc;
  if ((rc = assigned_offsets(c, cols, ncols, n, off)) != CQ_OK) return rc;
  for (size_t a = 0; a < ncols; a++)
    if (n && !out_dev[a]) return c->fail(CQ_ERR_ARG, "batch_invert_assigned: column " + std::to_string(a) + ": null output");
  if (!ncols || !n) return CQ_OK;
  const size_t total = off[ncols];
  HostStage st(c, 64 + round32(total * sizeof(uint32_t)) + total * sizeof(Fr), total * sizeof(Fr));
  if (st.rc != CQ_OK) return st.rc;
  uint32_t* verdict = (uint32_t*)st.din;
  uint32_t* rows = (uint32_t*)((char*)st.din + 64);
  Fr* den = (Fr*)((char*)rows + round32(total * sizeof(uint32_t)));
  std::vector<const Fr*> num(ncols);
  std::vector<Fr*> out(ncols);
  for (size_t a = 0; a < ncols; a++) {
    num[a] = (const Fr*)cols[a].num;
    out[a] = (Fr*)out_dev[a];
    if (!cols[a].den_count) continue;
    CQ_HIP(c, hipMemcpyAsync(rows + off[a], cols[a].den_rows, cols[a].den_count * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    CQ_HIP(c, hipMemcpyAsync(den + off[a], cols[a].den, cols[a].den_count * sizeof(Fr), hipMemcpyDeviceToDevice, c->stream));
  }
  if ((rc = poly_validate_assigned(c, off.data(), (uint32_t)ncols, rows, (uint32_t)n, verdict)) != CQ_OK) return rc;
  if ((rc = poly_resolve_assigned(c, num.data(), out.data(), off.data(), (uint32_t)ncols, rows, den, (uint32_t)n, (Fr*)st.dout, verdict)) != CQ_OK)
    return rc;
  uint32_t first_bad = 0;
  CQ_HIP(c, hipMemcpyAsync(&first_bad, verdict, sizeof(first_bad), hipMemcpyDeviceToHost, c->stream));
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  if (first_bad != 0xffffffffu) {
    size_t a = 0;
    while (a + 1 < ncols && off[a + 1] <= first_bad) a++;
    return c->fail(CQ_ERR_ARG, "batch_invert_assigned: column " + std::to_string(a) + ", entry " + std::to_string(first_bad - off[a]) +
                                   ": the row is not below n or does not ascend (nothing was written)");
  }
  return CQ_OK;
}

int cq_batch_invert_assigned(cq_ctx* c, const cq_assigned_column* cols, size_t ncols, size_t n, uint64_t* const* out_host) {
  if (!c || (ncols && (!cols || !out_host))) return CQ_ERR_ARG;
  CQ_HIP(c, hipSetDevice(c->device));
  std::vector<uint32_t> off;
  int rc;
  if ((rc = assigned_offsets(c, cols, ncols, n, off)) != CQ_OK) return rc;
  for (size_t a = 0; a < ncols; a++) {
    if (n && !out_host[a]) return c->fail(CQ_ERR_ARG, "batch_invert_assigned: column " + std::to_string(a) + ": null output");
    const size_t bad = assigned_rows_first_bad(cols[a].den_rows, cols[a].den_count, n);
    if (bad != cols[a].den_count)
      return c->fail(CQ_ERR_ARG, "batch_invert_assigned: column " + std::to_string(a) + ", entry " + std::to_string(bad) + ": row " +
                                     std::to_string(cols[a].den_rows[bad]) + " is not below n or does not ascend");
  }
  if (!ncols || !n) return CQ_OK;
  const size_t total = off[ncols], col_bytes = n * sizeof(Fr);
  HostStage st(c, ncols * col_bytes + round32(total * sizeof(uint32_t)) + total * sizeof(Fr), total * sizeof(Fr));
  if (st.rc != CQ_OK) return st.rc;
  uint32_t* rows = (uint32_t*)((char*)st.din + ncols * col_bytes);
  Fr* den = (Fr*)((char*)rows + round32(total * sizeof(uint32_t)));
  std::vector<const Fr*> num(ncols);
  std::vector<Fr*> out(ncols);
  for (size_t a = 0; a < ncols; a++) {
    out[a] = (Fr*)st.din + a * n;
    num[a] = out[a];
    CQ_HIP(c, hipMemcpyAsync(out[a], cols[a].num, col_bytes, hipMemcpyHostToDevice, c->stream));
    if (!cols[a].den_count) continue;
    CQ_HIP(c, hipMemcpyAsync(rows + off[a], cols[a].den_rows, cols[a].den_count * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    CQ_HIP(c, hipMemcpyAsync(den + off[a], cols[a].den, cols[a].den_count * sizeof(Fr), hipMemcpyHostToDevice, c->stream));
  }
  if ((rc = poly_resolve_assigned(c, num.data(), out.data(), off.data(), (uint32_t)ncols, rows, den, (uint32_t)n, (Fr*)st.dout, nullptr)) != CQ_OK)
    return rc;
  for (size_t a = 0; a < ncols; a++) CQ_HIP(c, hipMemcpyAsync(out_host[a], out[a], col_bytes, hipMemcpyDeviceToHost, c->stream));
  CQ_HIP(c, hipStreamSynchronize(c->stream));
  return CQ_OK;
}

}  // extern "C"

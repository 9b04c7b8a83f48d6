// Guard of the constructors behind the C ABI (capi_cq.hip, pk.hip).
#pragma once
#include <vector>
#include "ctx.hpp"
#include "msm.hpp"
#include "poly.hpp"

namespace cq {
// Owns a half-built object (and plain device allocations) until release(): every early return -- CQ_HIP included --
// destroys it, so a failing constructor leaks nothing and never hands back a live handle next to an error code.
template <class T>
struct Building {
  T* p;
  void (*destroy)(T*);
  std::vector<void*> dev;       // temporaries, hipFree'd on every path
  std::vector<const void*> reg; // temporary MSM window tables, unregistered on every path
  cq_ctx* c = nullptr;
  cq_domain* dom = nullptr;
  Building(T* p_, void (*d)(T*), cq_ctx* c_) : p(p_), destroy(d), c(c_) {}
  Building(const Building&) = delete;
  ~Building() {
    if (c) hipStreamSynchronize(c->stream);
    for (const void* r : reg) msm_unregister_tables(c, r);
    for (void* d : dev) hipFree(d);
    if (dom) domain_destroy(dom);
    if (p) destroy(p);
  }
  // a device temporary of `count` elements, freed with the guard
  template <class U>
  int temp(U** out, size_t count, const char* what) {
    int rc = c->dev_alloc(out, count, what);
    if (rc == CQ_OK) dev.push_back(*out);
    return rc;
  }
  // the finished object goes to the caller once the stream has drained
  int finish(T** out) {
    CQ_HIP(c, hipStreamSynchronize(c->stream));
    *out = release();
    return CQ_OK;
  }
  T* release() {
    T* q = p;
    p = nullptr;
    return q;
  }
};
}  // namespace cq

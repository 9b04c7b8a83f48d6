// Device helpers shared by the CQ kernels (cq.hip) and the witness checker (check.hip): 32-byte field loads / stores and
// the open-addressing value -> index hash of a static table (replaces BTreeMap<Fr, usize>, static_lookup.rs:72,82-85).
// `hash_fr` is a pure function of the eight words and also compiles without HIP (tests/host/tablehash_check.cpp).
#pragma once
#include "field.hpp"

namespace cq {

static CQ_HD uint32_t hash_fr(const Fr& v) {
  uint32_t h = 0x9e3779b9u;
  CQ_UNROLL
  for (int i = 0; i < 8; i++) {
    h ^= v.v.l[i];
    h *= 0x85ebca6bu;
    h ^= h >> 15;
  }
  return h;
}

#if defined(__HIPCC__)
static __device__ __forceinline__ Fr ld(const Fr* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  uint4 a = q[0], b = q[1];
  Fr r;
  r.v.l[0] = a.x; r.v.l[1] = a.y; r.v.l[2] = a.z; r.v.l[3] = a.w;
  r.v.l[4] = b.x; r.v.l[5] = b.y; r.v.l[6] = b.z; r.v.l[7] = b.w;
  return r;
}
static __device__ __forceinline__ void st(Fr* p, const Fr& r) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(r.v.l[0], r.v.l[1], r.v.l[2], r.v.l[3]);
  q[1] = make_uint4(r.v.l[4], r.v.l[5], r.v.l[6], r.v.l[7]);
}

constexpr uint32_t EMPTY = 0xffffffffu;

// slot array of `nslots` (power of two) table indices; values are compared in full (256 bits)
static __device__ __forceinline__ uint32_t table_find(const Fr* __restrict__ values, const uint32_t* __restrict__ slots,
                                                      uint32_t nslots, const Fr& v) {
  uint32_t s = hash_fr(v) & (nslots - 1);
  for (uint32_t probe = 0; probe < nslots; probe++) {
    const uint32_t idx = slots[s];
    if (idx == EMPTY) return EMPTY;
    if (ld(values + idx) == v) return idx;
    s = (s + 1) & (nslots - 1);
  }
  return EMPTY;
}
#endif  // __HIPCC__

}  // namespace cq

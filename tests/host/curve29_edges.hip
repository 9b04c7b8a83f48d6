// The G1 / G2 XYZZ group laws on the lazy limbs (curve29.hpp, curve2_29.hpp) on operands whose coordinates sit at the top
// of the headers' invariants, in several scalings of the same point; tests/test_field29_edges_gpu.py builds the records,
// runs them with
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -I sha2_on_cq_halo2_amd/csrc tests/host/curve29_edges.hip
//   curve29_edges IN OUT    -- IN: n records of REC_IN u32, OUT: n records of REC_OUT u32
// and compares the affine results with the Python group law.  A record: op, point A, point B, each as eight 9-limb values
// (G1 XYZZ: x y zz zzz; G1 affine: x y; G2 XYZZ: x.c0 x.c1 y.c0 ... zzz.c1; G2 affine: x.c0 x.c1 y.c0 y.c1).  The result
// is written in the XYZZ layout of its group.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include "curve2_29.hpp"
using namespace cq;

namespace {

constexpr int REC_IN = 1 + 2 * 72, REC_OUT = 72;
enum : uint32_t {
  G1_ADD, G1_ADD_AFFINE, G1_DBL, G1_DBL_AFFINE, G1_QUAD_ADD, G1_ADD_STORED,
  G2_ADD, G2_ADD_AFFINE, G2_DBL, G2_DBL_AFFINE, G2_ADD_STORED
};

__device__ Fq29 ld29(const uint32_t* p) {
  Fq29 r;
  for (int l = 0; l < 9; l++) r.a[l] = p[l];
  return r;
}
__device__ void st29(uint32_t* p, const Fq29& v) {
  for (int l = 0; l < 9; l++) p[l] = v.a[l];
}
__device__ XYZZ29 g1(const uint32_t* p) { return {ld29(p), ld29(p + 9), ld29(p + 18), ld29(p + 27)}; }
__device__ Affine29 g1a(const uint32_t* p) { return {ld29(p), ld29(p + 9)}; }
__device__ F2 f2(const uint32_t* p) { return {ld29(p), ld29(p + 9)}; }
__device__ XYZZ2_29 g2(const uint32_t* p) { return {f2(p), f2(p + 18), f2(p + 36), f2(p + 54)}; }
__device__ Affine2_29 g2a(const uint32_t* p) { return {f2(p), f2(p + 18)}; }
__device__ void put1(uint32_t* o, const XYZZ29& v) {
  st29(o, v.x);
  st29(o + 9, v.y);
  st29(o + 18, v.zz);
  st29(o + 27, v.zzz);
}
__device__ void put2(uint32_t* o, const XYZZ2_29& v) {
  const F2* c[4] = {&v.x, &v.y, &v.zz, &v.zzz};
  for (int k = 0; k < 4; k++) {
    st29(o + 18 * k, c[k]->c0);
    st29(o + 18 * k + 9, c[k]->c1);
  }
}

// one thread per record (every op but G1_QUAD_ADD); `scratch`: two memory-form points per record for the round trips
__global__ void serial_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, XYZZ2* __restrict__ scratch, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* r = in + (size_t)i * REC_IN;
  const uint32_t *a = r + 1, *b = r + 1 + 72;
  uint32_t* o = out + (size_t)i * REC_OUT;
  for (int l = 0; l < REC_OUT; l++) o[l] = 0;
  switch (r[0]) {
    case G1_ADD: { XYZZ29 acc = g1(a); xyzz29_add(acc, g1(b)); put1(o, acc); break; }
    case G1_ADD_AFFINE: { XYZZ29 acc = g1(a); xyzz29_add_affine(acc, g1a(b)); put1(o, acc); break; }
    case G1_DBL: put1(o, xyzz29_dbl(g1(a))); break;
    case G1_DBL_AFFINE: put1(o, xyzz29_dbl_affine(g1a(a))); break;
    case G1_ADD_STORED: {  // both operands through the memory form first (store reduces x: 8 p > 2^256)
      XYZZ* m = reinterpret_cast<XYZZ*>(scratch + 2 * (size_t)i);
      store_xyzz29(m, g1(a));
      store_xyzz29(m + 1, g1(b));
      XYZZ29 acc = load_xyzz29(m);
      xyzz29_add(acc, load_xyzz29(m + 1));
      put1(o, acc);
      break;
    }
    case G2_ADD: { XYZZ2_29 acc = g2(a); xyzz2_add(acc, g2(b)); put2(o, acc); break; }
    case G2_ADD_AFFINE: { XYZZ2_29 acc = g2(a); xyzz2_add_affine(acc, g2a(b)); put2(o, acc); break; }
    case G2_DBL: put2(o, xyzz2_dbl(g2(a))); break;
    case G2_DBL_AFFINE: put2(o, xyzz2_dbl_affine(g2a(a))); break;
    case G2_ADD_STORED: {
      XYZZ2* m = scratch + 2 * (size_t)i;
      store_xyzz2_29(m, g2(a));
      store_xyzz2_29(m + 1, g2(b));
      XYZZ2_29 acc = load_xyzz2_29(m);
      xyzz2_add(acc, load_xyzz2_29(m + 1));
      put2(o, acc);
      break;
    }
    default: o[0] = 0xffffffffu; break;
  }
}

// G1_QUAD_ADD: four lanes per record (the quads of a wave all execute quad_add: lanes past n add identities and write nothing)
__global__ __launch_bounds__(64) void quad_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
  const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x, i = lane >> 2, role = lane & 3u;
  const bool live = i < n;
  Fq29 F = Fq29::zero(), G = Fq29::zero();
  if (live) {
    const uint32_t* r = in + (size_t)i * REC_IN;
    F = ld29(r + 1 + 9 * role);
    G = ld29(r + 1 + 72 + 9 * role);
  }
  const Fq29 R = quad_add(F, G);
  if (live) st29(out + (size_t)i * REC_OUT + 9 * role, R);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint32_t> in;
  uint32_t buf[REC_IN];
  while (fread(buf, sizeof(uint32_t), REC_IN, f) == (size_t)REC_IN) in.insert(in.end(), buf, buf + REC_IN);
  fclose(f);
  const uint32_t n = (uint32_t)(in.size() / REC_IN);
  if (!n) return 2;
  // the quad records go to their own launch: split by op
  std::vector<uint32_t> qin, qidx, sin, sidx;
  for (uint32_t i = 0; i < n; i++) {
    const bool q = in[(size_t)i * REC_IN] == G1_QUAD_ADD;
    (q ? qin : sin).insert((q ? qin : sin).end(), in.begin() + (size_t)i * REC_IN, in.begin() + (size_t)(i + 1) * REC_IN);
    (q ? qidx : sidx).push_back(i);
  }
  std::vector<uint32_t> out((size_t)n * REC_OUT, 0);
  auto launch = [&](const std::vector<uint32_t>& hin, const std::vector<uint32_t>& idx, bool quad) -> bool {
    const uint32_t m = (uint32_t)idx.size();
    if (!m) return true;
    uint32_t *din = nullptr, *dout = nullptr;
    XYZZ2* scr = nullptr;
    if (hipMalloc(&din, hin.size() * 4) != hipSuccess || hipMalloc(&dout, (size_t)m * REC_OUT * 4) != hipSuccess ||
        hipMalloc(&scr, (size_t)m * 2 * sizeof(XYZZ2)) != hipSuccess ||
        hipMemcpy(din, hin.data(), hin.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
      return false;
    if (quad) quad_kernel<<<(unsigned)((4ull * m + 63) / 64), 64>>>(din, dout, m);
    else serial_kernel<<<(unsigned)((m + 63) / 64), 64>>>(din, dout, scr, m);
    std::vector<uint32_t> h((size_t)m * REC_OUT);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(h.data(), dout, h.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
      return false;
    for (uint32_t k = 0; k < m; k++)
      for (int l = 0; l < REC_OUT; l++) out[(size_t)idx[k] * REC_OUT + l] = h[(size_t)k * REC_OUT + l];
    (void)hipFree(din);
    (void)hipFree(dout);
    (void)hipFree(scr);
    return true;
  };
  if (!launch(sin, sidx, false) || !launch(qin, qidx, true)) {
    fprintf(stderr, "hip call failed\n");
    return 3;
  }
  FILE* g = fopen(argv[2], "wb");
  if (!g || fwrite(out.data(), 4, out.size(), g) != out.size()) return 2;
  fclose(g);
  printf("%u records\n", n);
  return 0;
}

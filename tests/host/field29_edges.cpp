// Edge-vector driver for the lazy 29-bit field types (field29.hpp Fp29 / Fq29 / Fr29, field2_29.hpp Fq2_29).
//
// Reads records of raw operand limbs, applies one named operation per record and writes the raw output limbs back; nothing
// is normalised or reduced by the driver.  The operands and the checks live in tests/field29_model.py.  One body, two builds:
//   host:   g++ -std=c++17 -I sha2_on_cq_halo2_amd/csrc tests/host/field29_edges.cpp            (tests/test_field29_edges_cpu.py)
//   device: hipcc --offload-arch=gfx950 -x hip ... (one thread per record; tests/test_field29_edges_gpu.py)
//   usage:  field29_edges IN OUT   -- IN: n records of REC_IN u32, OUT: n records of REC_OUT u32
#if !defined(__HIPCC__)
#define __device__
#define __forceinline__ inline
#endif
#include <cstdint>
#include <cstdio>
#include <vector>
#include "field2_29.hpp"

using namespace cq;

namespace {

constexpr int NOPS = 12;                  // operands per record (mac x 6: twelve)
constexpr int REC_IN = 1 + 9 * NOPS;      // op, then NOPS x 9 limbs
constexpr int REC_OUT = 32;               // up to three Fp29 results (27 u32), zero-padded

// op = (field << 8) | code, field 0 = Fq, 1 = Fr; codes 64.. are Fq2 operations (field 0 only).  Keep in step with
// tests/field29_model.py (OPS).
template <class P>
__device__ void apply_fp(uint32_t code, const uint32_t* in, uint32_t* out) {
  using F = Fp29<P>;
  F x[NOPS];
  for (int k = 0; k < NOPS; k++)
    for (int l = 0; l < 9; l++) x[k].a[l] = in[9 * k + l];
  F r[3] = {F::zero(), F::zero(), F::zero()};
  switch (code) {
    case 0: r[0] = F::mul(x[0], x[1]); break;
    case 1: r[0] = F::mul2(x[0], x[1], x[2], x[3]); break;
    case 2: case 3: case 4: case 5: case 6: case 7: {  // mac x n + redc, n = code - 1
      uint64_t c[18];
      for (int k = 0; k < 18; k++) c[k] = 0;
      for (uint32_t k = 0; k + 1 < code; k++) F::mac(c, x[2 * k], x[2 * k + 1]);
      r[0] = F::redc(c);
      break;
    }
    case 8: r[0] = x[0].sqr(); break;
    case 9: F::mul_pair(x[0], x[1], x[2], x[3], r[0], r[1]); break;
    case 10: F::sqr_pair(x[0], x[1], r[0], r[1]); break;
    case 11: F::mul2_mul_mul(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], r[0], r[1], r[2]); break;
    case 12: r[0] = F::template sub<2>(x[0], x[1]); break;
    case 13: r[0] = F::template sub<4>(x[0], x[1]); break;
    case 14: r[0] = F::template sub<8>(x[0], x[1]); break;
    case 15: r[0] = F::template sub<16>(x[0], x[1]); break;
    case 16: r[0] = F::template sub<32>(x[0], x[1]); break;
    case 17: r[0] = F::template sub<64>(x[0], x[1]); break;
    case 18: r[0] = F::template sub<6, 31>(x[0], x[1]); break;
    case 19: r[0] = F::template neg<2>(x[0]); break;
    case 20: r[0] = F::template neg<4>(x[0]); break;
    case 21: r[0] = x[0]; r[0].normalise(); break;
    case 22: r[0] = x[0].reduced(); break;
    case 23:
      r[0].a[0] = x[0].is_zero_mod_p() ? 1u : 0u;
      r[0].a[1] = x[0].limbs_zero() ? 1u : 0u;
      break;
    case 24: {
      uint32_t w[8];
      x[0].to_canonical_words(w);
      for (int l = 0; l < 8; l++) r[0].a[l] = w[l];
      break;
    }
    case 25: {
      const Fp<P> o = x[0].to_mont256();
      for (int l = 0; l < 8; l++) r[0].a[l] = o.v.l[l];
      break;
    }
    case 26: {  // the operand's first eight limbs are the eight words of an R = 2^256 value
      Fp<P> y;
      for (int l = 0; l < 8; l++) y.v.l[l] = in[l];
      r[0] = F::from_mont256(y);
      break;
    }
    case 27: {
      uint32_t w[8];
      x[0].pack(w);
      for (int l = 0; l < 8; l++) r[0].a[l] = w[l];
      break;
    }
    case 28: r[0] = F::unpack(in); break;
    case 29: {  // outputs aliasing the first operands, as the NTT's radix-4 step calls it
      r[0] = x[0];
      r[1] = x[2];
      F::mul_pair(r[0], x[1], r[1], x[3], r[0], r[1]);
      break;
    }
    case 30: {  // the second output aliasing y1 and x2, as the batch inversion calls it: mul_pair(b, r, r, e, o, r)
      r[1] = x[1];
      F::mul_pair(x[0], r[1], r[1], x[3], r[0], r[1]);
      break;
    }
    default: r[0].a[0] = 0xffffffffu; r[0].a[8] = 0xffffffffu; break;  // unknown op: a pattern no check accepts
  }
  for (int k = 0; k < 3; k++)
    for (int l = 0; l < 9; l++) out[9 * k + l] = r[k].a[l];
}

__device__ void apply_fq2(uint32_t code, const uint32_t* in, uint32_t* out) {
  Fq2_29 x[4];
  for (int k = 0; k < 4; k++)
    for (int l = 0; l < 9; l++) {
      x[k].c0.a[l] = in[18 * k + l];
      x[k].c1.a[l] = in[18 * k + 9 + l];
    }
  Fq2_29 r = Fq2_29::zero();
  switch (code) {
    case 64: r = Fq2_29::mul<2>(x[0], x[1]); break;
    case 65: r = Fq2_29::mul<6>(x[0], x[1]); break;
    case 66: r = x[0].sqr<2>(); break;
    case 67: r = x[0].sqr<4>(); break;
    case 68: r = Fq2_29::mul2<4, 2>(x[0], x[1], x[2], x[3]); break;
    default: r.c0.a[0] = 0xffffffffu; r.c0.a[8] = 0xffffffffu; break;
  }
  for (int l = 0; l < 9; l++) {
    out[l] = r.c0.a[l];
    out[9 + l] = r.c1.a[l];
  }
}

__device__ void apply(const uint32_t* in, uint32_t* out) {
  for (int l = 0; l < REC_OUT; l++) out[l] = 0;
  const uint32_t op = in[0], field = op >> 8, code = op & 0xffu;
  if (code >= 64 && field == 0) apply_fq2(code, in + 1, out);
  else if (field == 0) apply_fp<FqP>(code, in + 1, out);
  else apply_fp<FrP>(code, in + 1, out);
}

#if defined(__HIPCC__)
__global__ void edges_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  apply(in + (size_t)i * REC_IN, out + (size_t)i * REC_OUT);
}
#endif

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint32_t> in;
  uint32_t buf[REC_IN];
  while (fread(buf, sizeof(uint32_t), REC_IN, f) == (size_t)REC_IN) in.insert(in.end(), buf, buf + REC_IN);
  fclose(f);
  const size_t n = in.size() / REC_IN;
  std::vector<uint32_t> out(n * REC_OUT, 0);
#if defined(__HIPCC__)
  uint32_t *din = nullptr, *dout = nullptr;
  if (n && (hipMalloc(&din, in.size() * 4) != hipSuccess || hipMalloc(&dout, out.size() * 4) != hipSuccess ||
            hipMemcpy(din, in.data(), in.size() * 4, hipMemcpyHostToDevice) != hipSuccess)) {
    fprintf(stderr, "hip allocation / copy failed\n");
    return 3;
  }
  if (n) {
    edges_kernel<<<(unsigned)((n + 255) / 256), 256>>>(din, dout, (uint32_t)n);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(out.data(), dout, out.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) {
      fprintf(stderr, "kernel failed\n");
      return 3;
    }
    (void)hipFree(din);
    (void)hipFree(dout);
  }
#else
  for (size_t i = 0; i < n; i++) apply(in.data() + i * REC_IN, out.data() + i * REC_OUT);
#endif
  FILE* g = fopen(argv[2], "wb");
  if (!g || fwrite(out.data(), sizeof(uint32_t), out.size(), g) != out.size()) return 2;
  fclose(g);
  printf("%zu records\n", n);
  return 0;
}

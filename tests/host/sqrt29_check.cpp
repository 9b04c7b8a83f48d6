// Host driver for csrc/sqrt29.hpp (the Fq square root of point decompression), built with g++ the way field29_edges.cpp is:
//   g++ -std=c++17 -I sha2_on_cq_halo2_amd/csrc tests/host/sqrt29_check.cpp            (tests/test_serde_processed_cpu.py)
//   usage: sqrt29_check IN OUT   -- IN: n records of 9 u32 (the operand's limbs, R' = 2^261 Montgomery form, unreduced),
//                                   OUT: n records of REC_OUT u32:
//     [0..8)   canonical words of y = a^((q + 1) / 4)
//     [8]      sqrt_is_root29(y, a)
//     [9]      1 when every intermediate value had limbs 0..7 < 2^29
//     [10..19) the largest intermediate value (normalised limbs)
//     [19]     the number of intermediate values seen
//     [20..29) the root check's difference y^2 + 8 q - a (claimed < 10 q), its normalisation counted in [9]
// The operands and every check live in the Python test; nothing is judged here.
#define __device__
#define __forceinline__ inline
#include <cstdint>
#include <cstdio>
#include <vector>
#include "sqrt29.hpp"

using namespace cq;

namespace {

constexpr int REC_IN = 9, REC_OUT = 29;

struct MaxTrace {
  uint32_t max[9] = {};
  uint32_t normalised = 1, count = 0;
  uint32_t diff[9] = {};
  void difference(const Fq29& v) {
    for (int i = 0; i < 8; i++)
      if (v.a[i] >> 29) normalised = 0;
    for (int l = 0; l < 9; l++) diff[l] = v.a[l];
  }
  void operator()(const Fq29& v) {
    count++;
    for (int i = 0; i < 8; i++)
      if (v.a[i] >> 29) normalised = 0;
    for (int i = 8; i >= 0; i--) {  // normalised limbs compare like digits (a value that is not is reported above)
      if (v.a[i] == max[i]) continue;
      if (v.a[i] > max[i])
        for (int l = 0; l < 9; l++) max[l] = v.a[l];
      break;
    }
  }
};

void apply(const uint32_t* in, uint32_t* out) {
  Fq29 a;
  for (int l = 0; l < 9; l++) a.a[l] = in[l];
  MaxTrace tr;
  const Fq29 y = sqrt_candidate29<FqP, 4>(a, tr);
  out[8] = sqrt_is_root29<FqP>(y, a, tr) ? 1u : 0u;
  Fq29 lit1 = Fq29::zero();
  lit1.a[0] = 1;
  const Fq29 c = Fq29::mul(y, lit1);  // y R' * 1 / R' = y: out of Montgomery form, < 2 p
  c.pack(out);
  Fq::cond_sub_p(out, 0);
  out[9] = tr.normalised;
  for (int l = 0; l < 9; l++) out[10 + l] = tr.max[l];
  out[19] = tr.count;
  for (int l = 0; l < 9; l++) out[20 + l] = tr.diff[l];
}

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
  for (size_t i = 0; i < n; i++) apply(in.data() + i * REC_IN, out.data() + i * REC_OUT);
  FILE* g = fopen(argv[2], "wb");
  if (!g || fwrite(out.data(), sizeof(uint32_t), out.size(), g) != out.size()) return 2;
  fclose(g);
  printf("%zu records\n", n);
  return 0;
}

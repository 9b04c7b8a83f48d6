// Host driver for csrc/sqrt2_29.hpp (the Fq2 square root of G2 point decompression), built with g++ the way sqrt29_check.cpp is:
//   g++ -std=c++17 -I sha2_on_cq_halo2_amd/csrc tests/host/sqrt2_29_check.cpp           (tests/test_serde_g2_cpu.py)
//   usage: sqrt2_29_check IN OUT   -- IN: n records of 18 u32 (the limbs of a.c0 and a.c1, R' = 2^261 Montgomery form,
//                                     unreduced), OUT: n records of REC_OUT u32:
//     for ysign = 0 at [0..17), for ysign = 1 at [17..34):
//       [0..8) [8..16)  canonical words of the decoded y.c0, y.c1 (fq2_decoded_y29)
//       [16]            its verdict: a is a square
//     [34]      1 when every intermediate value of both runs had limbs 0..7 < 2^29
//     [35]      the number of intermediate values seen (both runs)
//     [36..45)  the largest value claimed < 2 q        [45..54) the largest claimed < 4 q
//     [54..63)  the largest claimed <= 2 q (negations)
// The operands and every check live in the Python test; nothing is judged here.
#define __device__
#define __forceinline__ inline
#include <cstdint>
#include <cstdio>
#include <vector>
#include "sqrt2_29.hpp"

using namespace cq;

namespace {

constexpr int REC_IN = 18, REC_OUT = 63;

struct MaxTrace {
  uint32_t max2[9] = {}, max4[9] = {}, maxn[9] = {};
  uint32_t normalised = 1, count = 0;
  void note(const Fq29& v, uint32_t* max) {
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
  void operator()(const Fq29& v) { note(v, max2); }
  void difference(const Fq29& v) { note(v, max4); }  // (sqrt29.hpp's root check: not used by the Fq2 route)
  void below4(const Fq29& v) { note(v, max4); }
  void negated(const Fq29& v) { note(v, maxn); }
};

void canonical(const Fq29& v, uint32_t* out) {
  Fq29 lit1 = Fq29::zero();
  lit1.a[0] = 1;
  const Fq29 c = Fq29::mul(v, lit1);  // v R' * 1 / R' = v: out of Montgomery form, < 2 q
  c.pack(out);
  Fq::cond_sub_p(out, 0);
}

void apply(const uint32_t* in, uint32_t* out) {
  Fq2_29 a;
  for (int l = 0; l < 9; l++) {
    a.c0.a[l] = in[l];
    a.c1.a[l] = in[9 + l];
  }
  MaxTrace tr;
  for (uint32_t ysign = 0; ysign < 2; ysign++) {
    Fq2_29 y;
    const bool sq = fq2_decoded_y29<4>(a, ysign, y, tr);
    uint32_t* o = out + 17 * ysign;
    canonical(y.c0, o);
    canonical(y.c1, o + 8);
    o[16] = sq ? 1u : 0u;
  }
  out[34] = tr.normalised;
  out[35] = tr.count;
  for (int l = 0; l < 9; l++) {
    out[36 + l] = tr.max2[l];
    out[45 + l] = tr.max4[l];
    out[54 + l] = tr.maxn[l];
  }
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

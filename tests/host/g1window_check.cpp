// Host driver for csrc/g1window.hpp (the signed-digit recoding behind the fixed-window G1 FFT), built with g++ and
// -fsanitize=address,undefined by tests/test_setup_powers_cpu.py:
//   usage: g1window_check IN OUT   -- IN: n records of 8 u32 (a canonical scalar k < r, low word first),
//                                     OUT: n records of REC_OUT u32:
//     [0..8)             the recoded words c
//     [8]                flip
//     [9 + 3 i + 0]      the window v_i of digit i < 85
//     [9 + 3 i + 1]      g1w_index(v_i)
//     [9 + 3 i + 2]      g1w_negative(v_i)
// The scalars and every check live in the Python test; nothing is judged here.
#define __device__
#define __forceinline__ inline
#include <cstdint>
#include <cstdio>
#include <vector>
#include "g1window.hpp"

using namespace cq;

namespace {
constexpr int REC_IN = 8, REC_OUT = 9 + 3 * G1W_DIGITS;
}

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
  for (size_t r = 0; r < n; r++) {
    const G1Recoded s = g1w_recode(in.data() + r * REC_IN);
    uint32_t* o = out.data() + r * REC_OUT;
    for (int i = 0; i < 8; i++) o[i] = s.c[i];
    o[8] = s.flip;
    for (int i = 0; i < G1W_DIGITS; i++) {
      const uint32_t v = g1w_window(s, i);
      o[9 + 3 * i] = v;
      o[9 + 3 * i + 1] = g1w_index(v);
      o[9 + 3 * i + 2] = g1w_negative(v) ? 1u : 0u;
    }
  }
  FILE* g = fopen(argv[2], "wb");
  if (!g || fwrite(out.data(), sizeof(uint32_t), out.size(), g) != out.size()) return 2;
  fclose(g);
  printf("%zu records\n", n);
  return 0;
}

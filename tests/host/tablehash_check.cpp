// HIP-free: tablehash.hpp's `hash_fr`, the value -> slot hash of a static table, on values given by the caller.  Reads field
// elements from standard input, eight hexadecimal 32-bit words each (the Montgomery form, least significant word first), and
// prints the hash of each, one hexadecimal word per line.  Built and run by tests/test_cq_round1_cpu.py, which compares the
// lines with tests/tablehash_model.py.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include "tablehash.hpp"

int main() {
  for (;;) {
    cq::Fr v;
    int got = 0;
    for (; got < 8; got++)
      if (scanf("%" SCNx32, &v.v.l[got]) != 1) break;
    if (got == 0) return 0;
    if (got != 8) {
      fprintf(stderr, "incomplete element: %d words\n", got);
      return 1;
    }
    printf("%08" PRIx32 "\n", cq::hash_fr(v));
  }
}

// Stand-alone host program for tests/test_assigned_cpu.py: runs the host validator of the Assigned column format
// (csrc/assigned_host.hpp) over row lists given on the command line, built with the host sanitizers.
//   assigned_rows <n> <limit> [row ...]   prints "<first bad entry or count> <entries below limit>"
// The list is copied into an exactly-sized heap block, so a read past either end is an AddressSanitizer report.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../sha2_on_cq_halo2_amd/csrc/assigned_host.hpp"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const size_t n = strtoull(argv[1], nullptr, 10), limit = strtoull(argv[2], nullptr, 10);
  const size_t count = (size_t)argc - 3;
  uint32_t* rows = count ? (uint32_t*)malloc(count * sizeof(uint32_t)) : nullptr;
  for (size_t i = 0; i < count; i++) rows[i] = (uint32_t)strtoul(argv[3 + i], nullptr, 10);
  const size_t bad = cq::assigned_rows_first_bad(rows, count, n);
  const size_t below = bad == count ? cq::assigned_rows_below(rows, count, limit) : 0;
  printf("%zu %zu\n", bad, below);
  free(rows);
  return 0;
}

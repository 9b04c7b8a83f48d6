// Host side of the Assigned column format (cq_assigned_column, include/cq_halo2.h): the check of a sparse row list that
// lies in host memory, O(den_count).  Plain C++ with no device code, so that tests/host/assigned_rows.cpp can run it
// under the host sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

namespace cq {

// A list is good when its rows ascend strictly and stay below n.  Returns the first entry that breaks that -- its row is
// not below n, or not above the row of the entry before it -- or `count` for a good list.
inline size_t assigned_rows_first_bad(const uint32_t* rows, size_t count, size_t n) {
  for (size_t i = 0; i < count; i++)
    if (rows[i] >= n || (i && rows[i - 1] >= rows[i])) return i;
  return count;
}

// how many entries of a good list name a row below `limit` (the list ascends: they are its head)
inline size_t assigned_rows_below(const uint32_t* rows, size_t count, size_t limit) {
  size_t lo = 0, hi = count;
  while (lo < hi) {
    const size_t mid = lo + (hi - lo) / 2;
    if (rows[mid] < limit) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

}  // namespace cq

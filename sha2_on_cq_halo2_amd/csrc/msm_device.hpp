// Device helpers that more than one translation unit of the G1 MSM engine needs (msm_sort.hip, msm_short.hip).  Every .hip
// file is compiled on its own without relocatable device code, so what kernels of two files share lives here, inlined.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace cq {

// exclusive scan of N (128 or 256) histogram bins by the first wave: lane l owns bins l * N/64 .. (l + 1) * N/64 - 1
template <uint32_t N>
static __device__ __forceinline__ void wave0_scan(const uint32_t* __restrict__ hist, uint32_t* __restrict__ start) {
  constexpr uint32_t PER = N / 64;
  const uint32_t l = threadIdx.x;
  if (l >= 64) return;
  uint32_t v[PER], sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < PER; k++) {
    v[k] = hist[PER * l + k];
    sum += v[k];
  }
  uint32_t incl = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(incl, d, 64);
    if ((int)l >= d) incl += o;
  }
  uint32_t run = incl - sum;
#pragma unroll
  for (uint32_t k = 0; k < PER; k++) {
    start[PER * l + k] = run;
    run += v[k];
  }
}

}  // namespace cq

// G1 MSM engine, step 3 of the pipeline (msm.hip has the overview): the plan -- exclusive scans of the bucket histogram that
// say where every bucket's entry list starts and how many bounded sub-lists it is cut into per level.  Every front
// (msm_sort.hip) runs it between its counting and its placing half.
#include "msm.hpp"

namespace cq {

// ---- 2. plan: exclusive scans over the flat bucket array -----------------------------------------
// Sequence 0 is the histogram itself (-> list start of every bucket); sequence k >= 1 is the
// number of level-k sub-lists of every bucket: t1 = ceil(cnt/S1); t_k = ceil(t_{k-1}/S2) while t_{k-1} > MSM_SHORT_MIN,
// else 0: a bucket with 2..MSM_SHORT_MIN partial sums is always finished by the lane groups of msm_combine_level_kernel,
// which are indexed by bucket and need no slot; one with a single partial sum was written to its bucket by the level
// before.  Lists of MSM_SHORT_MIN+1..MSM_SHORT partial sums own a slot (one wave) that is used only when the launch
// has few of them -- see combine_short_limit.
static __device__ __forceinline__ uint32_t level_value(uint32_t cnt, uint32_t lv, uint32_t s1) {
  if (lv == 0) return cnt;
  uint32_t t = (cnt + s1 - 1) / s1;
  for (uint32_t k = 2; k <= lv; k++) t = t <= MSM_SHORT_MIN ? 0 : (t + MSM_S2 - 1) / MSM_S2;
  return t;
}

// exclusive scan of one value per thread over a 256-thread block; returns prefix, total via out param
static __device__ __forceinline__ uint32_t block_excl_scan256(uint32_t v, uint32_t* sh /*>=4*/, uint32_t& total) {
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    uint32_t y = __shfl_up(x, off, 64);
    if ((int)lane >= off) x += y;
  }
  __syncthreads();
  if (lane == 63) sh[wid] = x;
  __syncthreads();
  uint32_t wbase = 0, tot = 0;
  for (uint32_t k = 0; k < 4; k++) {
    const uint32_t s = sh[k];
    if (k < wid) wbase += s;
    tot += s;
  }
  total = tot;
  return wbase + x - v;
}

constexpr uint32_t SCAN_TILE = 2048;  // elements per block (8 per thread)

__global__ __launch_bounds__(256) void msm_scan_reduce_kernel(const uint32_t* __restrict__ cnt, uint32_t Bt, uint32_t nseq, uint32_t s1,
                                                              const uint32_t* __restrict__ s1_dev /* the launch's own choice, or null */,
                                                              uint32_t* blocksums /*[nseq][nblk]*/, uint32_t* ticket) {
  CQ_CRITICAL_WAVES();
  __shared__ uint32_t sh[4];
  if (s1_dev) s1 = *s1_dev;
  const uint32_t base = blockIdx.x * SCAN_TILE + threadIdx.x * 8;
  uint32_t c8[8];
  for (int k = 0; k < 8; k++) c8[k] = (base + k < Bt) ? cnt[base + k] : 0;
  for (uint32_t lv = 0; lv < nseq; lv++) {
    uint32_t s = 0;
    for (int k = 0; k < 8; k++) s += level_value(c8[k], lv, s1);
    uint32_t tot;
    block_excl_scan256(s, sh, tot);
    if (threadIdx.x == 0) blocksums[(size_t)lv * gridDim.x + blockIdx.x] = tot;
  }
  // The block that finishes LAST turns the tile totals into exclusive offsets (what msm_scan_spine_kernel did in a launch of
  // its own, ~10 us of a front): a ticket per block behind a device-wide fence; the ticket word lies in the region the
  // launch's first kernel clears.
  __shared__ uint32_t last;
  __threadfence();
  if (threadIdx.x == 0) last = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
  __syncthreads();
  if (!last) return;
  __threadfence();
  const uint32_t nblk = gridDim.x;
  const uint32_t per = (nblk + 255) / 256;
  const uint32_t lo = min(threadIdx.x * per, nblk), hi = min(lo + per, nblk);
  for (uint32_t lv = 0; lv < nseq; lv++) {
    volatile uint32_t* a = blocksums + (size_t)lv * nblk;
    uint32_t s = 0;
    for (uint32_t j = lo; j < hi; j++) s += a[j];
    uint32_t tot;
    uint32_t run = block_excl_scan256(s, sh, tot);
    for (uint32_t j = lo; j < hi; j++) {
      const uint32_t v = a[j];
      a[j] = run;
      run += v;
    }
  }
}

__global__ __launch_bounds__(256) void msm_scan_apply_kernel(const uint32_t* __restrict__ cnt, uint32_t Bt, uint32_t nseq, uint32_t s1,
                                                             const uint32_t* __restrict__ s1_dev,
                                                             const uint32_t* __restrict__ blocksums,
                                                             uint32_t* __restrict__ off /*[nseq][Bt+1]*/,
                                                             uint32_t* __restrict__ tk /*[nseq-1][Bt]*/) {
  CQ_CRITICAL_WAVES();
  __shared__ uint32_t sh[4];
  if (s1_dev) s1 = *s1_dev;
  const uint32_t base = blockIdx.x * SCAN_TILE + threadIdx.x * 8;
  uint32_t c8[8];
  for (int k = 0; k < 8; k++) c8[k] = (base + k < Bt) ? cnt[base + k] : 0;
  for (uint32_t lv = 0; lv < nseq; lv++) {
    uint32_t v8[8];
    uint32_t s = 0;
    for (int k = 0; k < 8; k++) {
      v8[k] = level_value(c8[k], lv, s1);
      s += v8[k];
    }
    uint32_t tot;
    uint32_t run = block_excl_scan256(s, sh, tot) + blocksums[(size_t)lv * gridDim.x + blockIdx.x];
    uint32_t* o = off + (size_t)lv * (Bt + 1);
    for (int k = 0; k < 8; k++) {
      if (base + k < Bt) {
        o[base + k] = run;
        if (lv) tk[(size_t)(lv - 1) * Bt + base + k] = v8[k];
      }
      run += v8[k];
      if (base + k == Bt - 1) o[Bt] = run;
    }
  }
}

// s1_dev: the sub-list length the launch settled on (table and index fronts), or null for the host's s1
void msm_plan(hipStream_t s, const MsmLayout& L, const MsmBuffers& b, uint32_t s1, const uint32_t* s1_dev) {
  msm_scan_reduce_kernel<<<L.nblk, 256, 0, s>>>(b.counts, L.Bt, L.nseq, s1, s1_dev, b.blocksums, b.ticket);
  msm_scan_apply_kernel<<<L.nblk, 256, 0, s>>>(b.counts, L.Bt, L.nseq, s1, s1_dev, b.blocksums, b.off, b.tk);
}

}  // namespace cq

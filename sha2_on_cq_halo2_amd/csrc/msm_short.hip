// G1 MSM engine: the one-kernel short MSM (msm.hip has the overview of the generic pipeline this one skips).
#include "msm.hpp"
#include "msm_device.hpp"
#include "curve29.hpp"
#include "ctx.hpp"

namespace cq {

// ---- short plain-mode MSMs: one workgroup per (MSM, window) ---------------------------------------------------
// [b_0] and [p] of the CQ lookups are 2 L MSMs of N + 1 <= 2^12 + 1 terms over the proof's own bucket sums:
// 256 bucket sets of ~32 entries per bucket.  Through the generic pipeline that is eleven kernels built for 2^18-point
// launches, each waiting for the previous one's tail (0.8 ms at k = 18).  Here ONE launch does all of it, a 256-thread
// workgroup per (MSM, window) -- 8 x 32 = 256 workgroups, one per CU, a wave per SIMD:
//   0. digits : the canonical scalar + sum_w 128 * 256^w (below 2^256 for a scalar below r) has the bytes digit_w + 128 with
//               digit_w in [-128, 127]: every window independent of the others, no carry to hand on.  The workgroup keeps
//               the byte of ITS window per term (LDS, one byte each) and counts the 128 buckets |digit| - 1; equal keys of
//               a wave's leader are folded into one LDS atomic, so a vector of equal scalars costs an atomic per wave and
//               step, not one per entry.  Two MSMs over the same scalar vector ([b_0] and [p] of a lookup) each sort it
//               again: the sort is ~5 % of the workgroup's time, and one workgroup for both would leave half the CUs idle.
//   1. sums   : the E sorted entries (16 bits each: term | sign << 15) are cut into 256 segments of ceil(E / 256), one per lane,
//               whatever the buckets' sizes: every lane runs the same number of mixed additions (the launch is bound by
//               VALU issue: a wave takes as long as its longest lane).  A lane whose segment crosses into the next bucket
//               leaves the partial sum of the one it ends: lane t's partial sum of bucket b goes to slot t + b (strictly
//               increasing along the sorted order, at most 255 + 127), so a bucket's partial sums are adjacent slots.
//   2. buckets: two lanes per bucket add its <= SHORT_LONG partial sums (three, typically); the few buckets with more (a hot
//               bucket: equal scalars, 0 / 1 columns) go to a wave each: strided lane sums and a six-level shuffle tree.
//   3. planes : sum_d d B_d as the bit-plane sums of d - 1 and the plain total, by quads (quad_add: a chain of dependent
//               additions is what the workgroup waits for here).  Each wave sums two 64-bucket sets with sixteen quads --
//               waves 0..2 the planes w and w + 4, wave 3 plane 3 and its complement, whose sum is the total -- and writes
//               them where msm_weighted_kernel would: the host folds with msm_fold_windows as before.
// Sorted entries, partial sums and bucket sums live in the launch's workspace (64 KB + 2 n bytes per workgroup, L2-resident,
// written and read by the same workgroup); LDS holds the digit bytes and three 128-word tables only, so that a workgroup
// fits beside the four NTT pass workgroups a CU may hold for the side stream.
constexpr uint32_t SHORT_THREADS = 256, SHORT_BUCKETS = 128, SHORT_SLOTS = SHORT_THREADS + SHORT_BUCKETS, SHORT_LONG = 8;
static_assert(SHORT_THREADS == 2 * SHORT_BUCKETS, "two lanes per bucket in step 2");
static_assert(MSM_SHORT_LIMIT <= (1u << 15), "a sorted entry is 15 bits of term index and the sign");

static inline size_t short_ws_stride(uint32_t n) {
  return (((size_t)n * sizeof(uint16_t) + 255) & ~(size_t)255) + (size_t)(SHORT_SLOTS + SHORT_BUCKETS) * sizeof(XYZZ);
}

// One step of a counting sort's LDS atomics for a wave: returns the cell's value before this lane's entry.  The lanes that
// share the key of the first active lane are served by ONE atomic (their ranks follow from the ballot).
static __device__ __forceinline__ uint32_t short_rank(uint32_t* cells, bool act, uint32_t key, uint32_t lane) {
  uint32_t rank = 0;
  const unsigned long long pend = __ballot(act);
  if (pend) {  // wave-uniform
    const int leader = __ffsll((long long)pend) - 1;
    const uint32_t lkey = __shfl(key, leader, 64);
    const bool mine = act && key == lkey;
    const unsigned long long grp = __ballot(mine);
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(&cells[lkey], (uint32_t)__popcll(grp));
    base = __shfl(base, leader, 64);
    if (mine) rank = base + (uint32_t)__popcll(grp & ((1ull << lane) - 1ull));
    else if (act) rank = atomicAdd(&cells[key], 1u);
  }
  return rank;
}

__global__ __launch_bounds__(SHORT_THREADS) void msm_short_kernel(MsmPtrs sc, MsmPtrs bs, uint32_t n, char* __restrict__ ws, size_t ws_stride,
                                                                  G1Jac* __restrict__ out) {
  CQ_CRITICAL_WAVES();
  extern __shared__ uint8_t dig[];  // n bytes: digit + 128 of this window, per term
  __shared__ uint32_t hist[SHORT_BUCKETS], cursor[SHORT_BUCKETS], bstart[SHORT_BUCKETS + 1];
  const uint32_t w = blockIdx.x, m = blockIdx.y, t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  const Fr* __restrict__ scal = (const Fr*)sc.p[m];
  const G1Affine* __restrict__ pts = (const G1Affine*)bs.p[m];
  char* mine_ws = ws + ((size_t)m * MSM_SHORT_W + w) * ws_stride;
  uint16_t* sorted = (uint16_t*)mine_ws;
  XYZZ* slots = (XYZZ*)(mine_ws + (((size_t)n * sizeof(uint16_t) + 255) & ~(size_t)255));
  XYZZ* bk = slots + SHORT_SLOTS;
  // bucket |digit| - 1 of a byte that is not 128 (digit = byte - 128)
  auto key_of = [](uint32_t byte) { return byte > 128u ? byte - 129u : 127u - byte; };

  // ---- 0. digits, counting sort ----
  if (t < SHORT_BUCKETS) {
    hist[t] = 0;
    cursor[t] = 0;
  }
  __syncthreads();
#pragma unroll 1
  for (uint32_t i0 = 0; i0 < n; i0 += SHORT_THREADS) {  // (the same trip count for every lane: the ballots need whole waves)
    const uint32_t i = i0 + t;
    uint32_t byte = 128;
    if (i < n) {
      U256 v = scal[i].to_canonical();
      uint32_t carry = 0, limb = 0;
      CQ_UNROLL for (int k = 0; k < 8; k++) {
        const uint64_t s = (uint64_t)v.l[k] + 0x80808080u + carry;
        carry = (uint32_t)(s >> 32);
        limb = (w >> 2) == (uint32_t)k ? (uint32_t)s : limb;  // (no run-time index into v: that would put it in scratch memory)
      }
      byte = (limb >> (8 * (w & 3u))) & 0xffu;
      dig[i] = (uint8_t)byte;
    }
    (void)short_rank(hist, byte != 128u, key_of(byte) & 127u, lane);
  }
  __syncthreads();
  wave0_scan<SHORT_BUCKETS>(hist, bstart);
  __syncthreads();
  if (t == 0) bstart[SHORT_BUCKETS] = bstart[SHORT_BUCKETS - 1] + hist[SHORT_BUCKETS - 1];
#pragma unroll 1
  for (uint32_t i0 = 0; i0 < n; i0 += SHORT_THREADS) {
    const uint32_t i = i0 + t;
    const uint32_t byte = i < n ? dig[i] : 128u;  // (written by this very lane above)
    const bool act = byte != 128u;
    const uint32_t key = key_of(byte) & 127u;
    const uint32_t rank = short_rank(cursor, act, key, lane);
    if (act) sorted[bstart[key] + rank] = (uint16_t)(i | (byte < 128u ? 0x8000u : 0u));
  }
  __syncthreads();

  // ---- 1. one segment of the sorted entries per lane ----
  const uint32_t E = bstart[SHORT_BUCKETS];
  const uint32_t per = (E + SHORT_THREADS - 1) / SHORT_THREADS;
  const uint32_t lo = min(t * per, E), hi = min(lo + per, E);
  if (lo < hi) {
    uint32_t b = 0;
    {
      uint32_t l = 0, h = SHORT_BUCKETS;  // bstart[l] <= lo < bstart[h]: the last such l is the bucket that holds entry lo
      while (h - l > 1) {
        const uint32_t mid = (l + h) >> 1;
        if (bstart[mid] <= lo) l = mid; else h = mid;
      }
      b = l;
    }
    uint32_t bend = bstart[b + 1];
    XYZZ29 acc = XYZZ29::identity();
    // (the pipeline of msm_accumulate_kernel: the next point's gather is in flight while the current one is added)
    uint32_t ix_cur = sorted[lo];
    uint32_t ix_next = lo + 1 < hi ? sorted[lo + 1] : 0u;
    uint32_t wx[8], wy[8];
    {
      const G1Affine* q = pts + (ix_cur & 0x7fffu);
      ld8(&q->x, wx);
      ld8(&q->y, wy);
    }
#pragma unroll 1
    for (uint32_t e = lo; e < hi; e++) {
      if (e >= bend) {  // bucket b ends inside this segment: its partial sum leaves, the next non-empty bucket begins
        store_xyzz29(slots + t + b, acc);
        acc = XYZZ29::identity();
        do {
          b++;
          bend = bstart[b + 1];
        } while (e >= bend);
      }
      Affine29 p;
      p.x = Fq29::unpack(wx);
      p.y = Fq29::unpack(wy);
      const uint32_t neg = ix_cur >> 15;
      ix_cur = ix_next;
      if (e + 1 < hi) {
        const G1Affine* q = pts + (ix_cur & 0x7fffu);
        ld8(&q->x, wx);
        ld8(&q->y, wy);
      }
      ix_next = e + 2 < hi ? sorted[e + 2] : 0u;
      {  // R = 2^256 values of the caller's array
        Fq29 f;
        CQ_UNROLL for (int i = 0; i < 9; i++) f.a[i] = CONSTS29<FqP>.from256[i];
        Fq29::mul_pair(p.x, f, p.y, f, p.x, p.y);
      }
      if (neg && !p.is_identity()) p.y = Fq29::neg<2>(p.y);
      xyzz29_add_affine(acc, p);
    }
    store_xyzz29(slots + t + b, acc);
  }
  __syncthreads();

  // ---- 2. bucket sums: the lanes s0 / per .. (s1 - 1) / per hold entries of a bucket whose list is [s0, s1) ----
  {
    const uint32_t b = t >> 1, sub = t & 1u;
    const uint32_t s0 = bstart[b], s1 = bstart[b + 1];
    const uint32_t tlo = s1 > s0 ? s0 / per : 0u;
    const uint32_t parts = s1 > s0 ? (s1 - 1) / per - tlo + 1 : 0u;
    const bool own = parts <= SHORT_LONG;  // (an empty bucket as well: it is written as the identity)
    XYZZ29 acc = XYZZ29::identity();
    if (own) {
#pragma unroll 1
      for (uint32_t j = sub; j < parts; j += 2) xyzz29_add(acc, load_xyzz29(slots + tlo + j + b));
    }
    xyzz29_tree_sum<2>(acc, sub, own);
    if (own && sub == 0) store_xyzz29(bk + b, acc);
  }
  {
    uint32_t nlong = 0;
#pragma unroll 1
    for (uint32_t b = 0; b < SHORT_BUCKETS; b++) {  // (every test below is wave-uniform)
      const uint32_t s0 = bstart[b], s1 = bstart[b + 1];
      if (s1 <= s0) continue;
      const uint32_t tlo = s0 / per, parts = (s1 - 1) / per - tlo + 1;
      if (parts <= SHORT_LONG) continue;
      if ((nlong++ & 3u) != wave) continue;
      XYZZ29 acc = XYZZ29::identity();
#pragma unroll 1
      for (uint32_t j = lane; j < parts; j += 64) xyzz29_add(acc, load_xyzz29(slots + tlo + j + b));
      xyzz29_tree_sum<64>(acc, lane);
      if (lane == 0) store_xyzz29(bk + b, acc);
    }
  }
  __syncthreads();

  // ---- 3. bit planes of d - 1 and the total, sixteen quads per wave (lane r of a quad: coordinate r) ----
  const uint32_t role = t & 3u, quad = lane >> 2;
  G1Jac* o = out + ((size_t)m * MSM_SHORT_W + w) * MSM_SET_POINTS;
  Fq29 first = Fq29::zero();
#pragma unroll 1
  for (uint32_t rep = 0; rep < 2; rep++) {
    // the 64 buckets whose index has bit `tb` set (clear, for wave 3's second set)
    const uint32_t tb = rep == 0 ? wave : wave < 3 ? wave + 4 : 3u;
    const uint32_t bit = rep == 1 && wave == 3 ? 0u : 1u << tb;
    auto index = [&](uint32_t j) { return ((j >> tb) << (tb + 1)) | bit | (j & ((1u << tb) - 1u)); };
    Fq29 F = quad_load(bk + index(quad), role);
#pragma unroll 1
    for (uint32_t k = 1; k < 4; k++) F = quad_add(F, quad_load(bk + index(quad + 16 * k), role));
    F = quad_wave_sum(F, 32);
    if (rep == 0) first = F;
    else if (wave == 3) F = quad_add(first, F);  // plane 3 + its complement: the total
    const uint32_t slot = rep == 0 ? 7 + wave : wave < 3 ? 11 + wave : MSM_SET_POINTS - 1;
    const XYZZ29 v = quad_to_xyzz29(F);
    if (lane == 0) o[slot] = xyzz29_to_jac(v);
  }
}

size_t msm_short_workspace(uint32_t n, uint32_t batch) { return short_ws_stride(n) * MSM_SHORT_W * batch; }

int msm_short_run(cq_ctx* ctx, const Fr* const* scalars, const G1Affine* const* bases, uint32_t n, uint32_t batch, void* workspace,
                  G1Jac* window_sums_dev) {
  if (!batch || batch > MSM_MAX_BATCH || !n || n > MSM_SHORT_LIMIT) return -2;
  MsmPtrs sp, bp;
  for (uint32_t i = 0; i < MSM_MAX_BATCH; i++) {
    sp.p[i] = i < batch ? (const void*)scalars[i] : nullptr;
    bp.p[i] = i < batch ? (const void*)bases[i] : nullptr;
  }
  const size_t lds = ((size_t)n + 15) & ~(size_t)15;
  msm_short_kernel<<<dim3(MSM_SHORT_W, batch), SHORT_THREADS, lds, ctx->stream>>>(sp, bp, n, (char*)workspace, short_ws_stride(n),
                                                                                 window_sums_dev);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace cq

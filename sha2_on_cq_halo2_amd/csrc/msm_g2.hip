// G2 multi-scalar multiplication (`best_multiexp` over G2Affine, arithmetic.rs:132-159) and the G2 powers of the test
// SRS (the `g2` vector of TableSRS::setup_from_toxic_waste, poly/kzg/commitment.rs:73-123).
//
// A self-contained Pippenger: the G1 engine (msm.hip) is tuned around 64-byte points and its window tables, and none of
// its kernels is shared, so the G1 proof path keeps its code objects.  One-shot use (keygen), so no window tables here.
//   1. digits: canonical scalars; signed c-bit digits (2^(c-1) buckets per window, W = ceil(255 / c) windows);
//   2. counting sort of the (scalar, window) entries by bucket: a histogram (atomics), one scan, a scatter;
//   3. bucket sums in levels: level 1 gives every lane at most G2_S1 entries of ONE bucket (mixed additions of the
//      affine bases); level L >= 2 sums at most G2_S partial sums of the previous level per lane -- until every bucket
//      has one value.  A bucket's lanes never depend on its length, so repeated bases and scalars cost no more than
//      random ones;
//   4. window sums: each lane takes G2_RED consecutive buckets (running sum), adds k * (their sum) for its offset k by
//      double-and-add, and groups of G2_S lanes' results are summed in a tree;
//   5. the host folds the W window sums (c doublings each).
// Every kernel keeps its G2 accumulator (8 Fq = 72 VGPRs in limb form) in registers: see DESIGN.md for the figures.
#include <algorithm>
#include <vector>
#include "ctx.hpp"
#include "curve2_29.hpp"
#include "msm_g2.hpp"

namespace cq {

namespace {

constexpr uint32_t G2_S1 = 32;          // entries per lane, level 1
constexpr uint32_t G2_S = 16;           // partial sums per lane, levels >= 2 and the window tree
constexpr uint32_t G2_RED = 16;         // buckets per lane of the window reduction
constexpr uint32_t G2_THREADS = 128;    // lanes per block of the addition kernels
constexpr uint32_t G2_MAX_LEVELS = 8;

// ---- 1. digits ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void g2_canon_kernel(const Fr* __restrict__ scalars, uint32_t n, U256* __restrict__ canon) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  canon[i] = scalars[i].to_canonical();
}

// bits [off, off + c) of a canonical scalar (off < 256, c <= 16); read from memory, so the index may vary
static __device__ __forceinline__ uint32_t window_bits(const U256* __restrict__ canon, uint32_t i, uint32_t off, uint32_t c) {
  const uint32_t* w = canon[i].l;
  const uint32_t li = off >> 5, sh = off & 31;
  const uint64_t lo = w[li], hi = li + 1 < 8 ? w[li + 1] : 0u;
  return (uint32_t)(((hi << 32) | lo) >> sh) & ((1u << c) - 1u);
}

// signed digit of window w, given the carry of window w - 1: in (-2^(c-1), 2^(c-1)], as magnitude and sign
static __device__ __forceinline__ uint32_t next_digit(uint32_t raw, uint32_t c, uint32_t& carry, uint32_t& neg) {
  const uint32_t half = 1u << (c - 1);
  const uint32_t v = raw + carry;
  if (v > half) {
    carry = 1;
    neg = 1;
    return (1u << c) - v;  // 0 when v == 2^c
  }
  carry = 0;
  neg = 0;
  return v;
}

// ---- 2. counting sort --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void g2_count_kernel(const U256* __restrict__ canon, uint32_t n, uint32_t c, uint32_t W,
                                                       uint32_t* __restrict__ counts) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t M = 1u << (c - 1);
  uint32_t carry = 0, neg;
  for (uint32_t w = 0; w < W; w++) {
    const uint32_t d = next_digit(window_bits(canon, i, w * c, c), c, carry, neg);
    if (d) atomicAdd(&counts[w * M + d - 1], 1u);
  }
}

// off[b] = sum_{b' < b} ceil(counts[b'] / D) for b <= B (off[B] = the total); one block
__global__ __launch_bounds__(1024) void g2_scan_kernel(const uint32_t* __restrict__ counts, uint32_t B, uint64_t D,
                                                       uint32_t* __restrict__ off) {
  __shared__ uint32_t sh[1024];
  const uint32_t t = threadIdx.x, per = (B + 1023) / 1024;
  const uint32_t lo = min(B, t * per), hi = min(B, lo + per);
  uint32_t s = 0;
  for (uint32_t b = lo; b < hi; b++) s += (uint32_t)((counts[b] + D - 1) / D);
  sh[t] = s;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {
    const uint32_t v = t >= d ? sh[t - d] : 0u;
    __syncthreads();
    sh[t] += v;
    __syncthreads();
  }
  uint32_t run = sh[t] - s;
  for (uint32_t b = lo; b < hi; b++) {
    off[b] = run;
    run += (uint32_t)((counts[b] + D - 1) / D);
  }
  if (t == 1023) off[B] = sh[1023];
}

// entries: scalar index | sign << 31, grouped by bucket (order inside a bucket: arrival)
__global__ __launch_bounds__(256) void g2_scatter_kernel(const U256* __restrict__ canon, uint32_t n, uint32_t c, uint32_t W,
                                                         const uint32_t* __restrict__ off, uint32_t* __restrict__ cursor,
                                                         uint32_t* __restrict__ entries) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t M = 1u << (c - 1);
  uint32_t carry = 0, neg;
  for (uint32_t w = 0; w < W; w++) {
    const uint32_t d = next_digit(window_bits(canon, i, w * c, c), c, carry, neg);
    if (d) {
      const uint32_t b = w * M + d - 1;
      entries[off[b] + atomicAdd(&cursor[b], 1u)] = i | (neg << 31);
    }
  }
}

// ---- 3. bucket sums ----------------------------------------------------------------------------------------------
// the bucket whose range [off[b], off[b + 1]) holds item t (off non-decreasing, off[B] > t)
static __device__ __forceinline__ uint32_t owner(const uint32_t* __restrict__ off, uint32_t B, uint32_t t) {
  uint32_t lo = 0, hi = B - 1;  // the largest b with off[b] <= t
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (off[mid] <= t) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(G2_THREADS) void g2_bucket_level1_kernel(const uint32_t* __restrict__ entries, const uint32_t* __restrict__ off0,
                                                                       const uint32_t* __restrict__ off1, uint32_t B,
                                                                       const G2Affine* __restrict__ bases, XYZZ2* __restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= off1[B]) return;
  const uint32_t b = owner(off1, B, t);
  const uint32_t lo = off0[b] + (t - off1[b]) * G2_S1, hi = min(off0[b + 1], lo + G2_S1);
  XYZZ2_29 acc = XYZZ2_29::identity();
  for (uint32_t e = lo; e < hi; e++) {
    const uint32_t v = entries[e];
    Affine2_29 a = load_affine2_29(bases + (v & 0x7fffffffu));
    if (a.is_identity()) continue;
    if (v >> 31) a.y = F2::neg<2>(a.y);
    xyzz2_add_affine(acc, a);
  }
  store_xyzz2_29(out + t, acc);
}

__global__ __launch_bounds__(G2_THREADS) void g2_bucket_level_kernel(const XYZZ2* __restrict__ in, const uint32_t* __restrict__ off_in,
                                                                      const uint32_t* __restrict__ off_out, uint32_t B,
                                                                      XYZZ2* __restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= off_out[B]) return;
  const uint32_t b = owner(off_out, B, t);
  const uint32_t lo = off_in[b] + (t - off_out[b]) * G2_S, hi = min(off_in[b + 1], lo + G2_S);
  XYZZ2_29 acc = load_xyzz2_29(in + lo);
  for (uint32_t e = lo + 1; e < hi; e++) xyzz2_add(acc, load_xyzz2_29(in + e));
  store_xyzz2_29(out + t, acc);
}

// ---- 4. window sums ----------------------------------------------------------------------------------------------
// lane (w, g) of G per window: buckets d = g R + 1 .. (g + 1) R of window w (value of bucket b: its one item of the last
// level, or the identity).  Writes sum_d d * S_d over its buckets = sum_d (d - g R) S_d + g R * sum_d S_d.
__global__ __launch_bounds__(G2_THREADS) void g2_window_reduce_kernel(const XYZZ2* __restrict__ items, const uint32_t* __restrict__ off,
                                                                       uint32_t M, uint32_t W, uint32_t G, uint32_t R,
                                                                       XYZZ2* __restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= W * G) return;
  const uint32_t w = t / G, g = t % G;
  XYZZ2_29 run = XYZZ2_29::identity(), acc = XYZZ2_29::identity();
  for (uint32_t d = (g + 1) * R; d > g * R; d--) {
    const uint32_t b = w * M + d - 1;
    if (off[b + 1] > off[b]) xyzz2_add(run, load_xyzz2_29(items + off[b]));
    xyzz2_add(acc, run);
  }
  // + (g R) * run, double-and-add (g R < M <= 2^15)
  for (uint32_t k = g * R; k; k >>= 1) {
    if (k & 1) xyzz2_add(acc, run);
    if (k > 1) run = xyzz2_dbl(run);
  }
  store_xyzz2_29(out + t, acc);
}

// out[t] = sum of in[t * S .. min((t + 1) * S, n))
__global__ __launch_bounds__(G2_THREADS) void g2_sum_groups_kernel(const XYZZ2* __restrict__ in, uint32_t n, uint32_t S,
                                                                    XYZZ2* __restrict__ out, uint32_t nout) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nout) return;
  const uint32_t lo = t * S, hi = min(n, lo + S);
  XYZZ2_29 acc = XYZZ2_29::identity();
  for (uint32_t e = lo; e < hi; e++) xyzz2_add(acc, load_xyzz2_29(in + e));
  store_xyzz2_29(out + t, acc);
}

__global__ __launch_bounds__(64) void g2_to_jac_kernel(const XYZZ2* __restrict__ in, uint32_t n, G2Jac* __restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  out[t] = xyzz2_to_jac(load_xyzz2_29(in + t));
}

// ---- SRS powers: fixed-base multiplication by a host-built table T[j][d] = d * 2^(8j) * G2 -------------------------
__global__ __launch_bounds__(G2_THREADS) void g2_fixed_base_powers_kernel(Fr s, uint32_t count, const G2Affine* __restrict__ table,
                                                                           G2Affine* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const U256 v = s.pow_u64(i).to_canonical();
  XYZZ2_29 acc = XYZZ2_29::identity();
  for (uint32_t j = 0; j < 32; j++) {
    const uint32_t byte = (v.l[j >> 2] >> ((j & 3) * 8)) & 0xffu;
    if (byte) xyzz2_add_affine(acc, load_affine2_29(table + j * 256 + byte));
  }
  G2Affine r = G2Affine::identity();
  if (!acc.is_identity()) {  // x = X / ZZ, y = Y / ZZZ with one Fq2 inversion of ZZ ZZZ (one Fq inversion of its norm)
    const Fq2 x = to_mont256_2(acc.x), y = to_mont256_2(acc.y), zz = to_mont256_2(acc.zz), zzz = to_mont256_2(acc.zzz);
    const Fq2 iv = (zz * zzz).inv();
    r.x = x * (iv * zzz);
    r.y = y * (iv * zz);
  }
  out[i] = r;
}

}  // namespace

uint32_t g2_msm_window_bits(size_t n) {
  uint32_t lg = 0;
  while (((size_t)1 << (lg + 1)) <= n) lg++;
  return lg < 8 ? 4 : lg > 20 ? 16 : lg - 4;
}

int g2_msm(cq_ctx* c, const Fr* scalars_dev, const G2Affine* bases_dev, size_t n_, G2Jac* out) {
  *out = G2Jac::identity();
  if (n_ == 0) return CQ_OK;
  const uint32_t cb = g2_msm_window_bits(n_), W = (255 + cb - 1) / cb, M = 1u << (cb - 1), B = W * M;
  // entry indices hold 31 bits and bucket offsets 32
  if (n_ >= (1u << 31) || (uint64_t)n_ * W >= ((uint64_t)1 << 32)) return c->fail(CQ_ERR_ARG, "g2 msm: too many terms");
  hipStream_t st = c->stream;
  const uint32_t n = (uint32_t)n_;
  // levels: divisor D_L = G2_S1 * G2_S^(L-1) until it covers the longest possible bucket (n entries)
  uint64_t D[G2_MAX_LEVELS];
  uint32_t L = 0;
  for (uint64_t d = G2_S1;; d *= G2_S) {
    D[L++] = d;
    if (d >= n || L == G2_MAX_LEVELS) break;
  }
  const uint64_t entries = (uint64_t)n * W;
  auto bound = [&](uint32_t l) { return (entries + D[l] - 1) / D[l] + B; };  // items of level l + 1
  const uint64_t capA = bound(0), capB = L > 1 ? bound(1) : 1;
  const uint32_t R = std::min(G2_RED, M), G = M / R;
  // workspace
  const size_t sz_canon = (size_t)n * sizeof(U256), sz_ent = entries * 4, sz_cnt = (size_t)B * 4, sz_off = (size_t)(L + 1) * (B + 1) * 4;
  const size_t sz_a = capA * sizeof(XYZZ2), sz_b = capB * sizeof(XYZZ2), sz_red = (size_t)2 * W * G * sizeof(XYZZ2), sz_jac = (size_t)W * sizeof(G2Jac);
  size_t offs[9], total = 0;
  const size_t sizes[9] = {sz_canon, sz_ent, sz_cnt, sz_cnt, sz_off, sz_a, sz_b, sz_red, sz_jac};
  for (int i = 0; i < 9; i++) {
    offs[i] = total;
    total += (sizes[i] + 255) & ~(size_t)255;
  }
  char* ws = nullptr;
  CQ_HIP(c, hipMalloc(&ws, total));
  struct Free {
    char* p;
    hipStream_t s;
    ~Free() {
      hipStreamSynchronize(s);
      hipFree(p);
    }
  } guard{ws, st};
  U256* canon = (U256*)(ws + offs[0]);
  uint32_t* ent = (uint32_t*)(ws + offs[1]);
  uint32_t* counts = (uint32_t*)(ws + offs[2]);
  uint32_t* cursor = (uint32_t*)(ws + offs[3]);
  uint32_t* off = (uint32_t*)(ws + offs[4]);  // off + l (B + 1): level l (0 = entries)
  XYZZ2* part[2] = {(XYZZ2*)(ws + offs[5]), (XYZZ2*)(ws + offs[6])};
  XYZZ2* red = (XYZZ2*)(ws + offs[7]);
  G2Jac* jac = (G2Jac*)(ws + offs[8]);
  const uint32_t nb = (n + 255) / 256;
  auto blocks = [](uint64_t lanes) { return (uint32_t)((lanes + G2_THREADS - 1) / G2_THREADS); };

  CQ_HIP(c, hipMemsetAsync(counts, 0, 2 * ((sz_cnt + 255) & ~(size_t)255), st));  // counts and cursor
  g2_canon_kernel<<<nb, 256, 0, st>>>(scalars_dev, n, canon);
  g2_count_kernel<<<nb, 256, 0, st>>>(canon, n, cb, W, counts);
  for (uint32_t l = 0; l <= L; l++) g2_scan_kernel<<<1, 1024, 0, st>>>(counts, B, l ? D[l - 1] : 1, off + (size_t)l * (B + 1));
  g2_scatter_kernel<<<nb, 256, 0, st>>>(canon, n, cb, W, off, cursor, ent);
  g2_bucket_level1_kernel<<<blocks(capA), G2_THREADS, 0, st>>>(ent, off, off + (B + 1), B, bases_dev, part[0]);
  for (uint32_t l = 1; l < L; l++)
    g2_bucket_level_kernel<<<blocks(bound(l)), G2_THREADS, 0, st>>>(part[(l - 1) & 1], off + (size_t)l * (B + 1),
                                                                    off + (size_t)(l + 1) * (B + 1), B, part[l & 1]);
  XYZZ2* items = part[(L - 1) & 1];
  g2_window_reduce_kernel<<<blocks((uint64_t)W * G), G2_THREADS, 0, st>>>(items, off + (size_t)L * (B + 1), M, W, G, R, red);
  // G lanes per window -> 1, in groups of G2_S (G is a power of two, so groups never straddle windows)
  XYZZ2* src = red;
  XYZZ2* dst = red + (size_t)W * G;
  for (uint32_t g = G; g > 1;) {
    const uint32_t s = std::min(G2_S, g), ng = g / s;
    g2_sum_groups_kernel<<<blocks((uint64_t)W * ng), G2_THREADS, 0, st>>>(src, W * g, s, dst, W * ng);
    std::swap(src, dst);
    g = ng;
  }
  g2_to_jac_kernel<<<(W + 63) / 64, 64, 0, st>>>(src, W, jac);
  CQ_HIP(c, hipGetLastError());
  std::vector<G2Jac> win(W);
  CQ_HIP(c, hipMemcpyAsync(win.data(), jac, sz_jac, hipMemcpyDeviceToHost, st));
  CQ_HIP(c, hipStreamSynchronize(st));
  G2Jac acc = G2Jac::identity();
  for (uint32_t w = W; w-- > 0;) {
    for (uint32_t k = 0; k < cb; k++) acc = g2_jac_dbl(acc);
    acc = g2_jac_add(acc, win[w]);
  }
  *out = acc;
  return CQ_OK;
}

int g2_srs_powers(cq_ctx* c, const Fr& s, uint32_t count, G2Affine* out_dev) {
  if (count == 0) return CQ_OK;
  // host: T[j][d] = d * 2^(8j) * G2, normalised with one inversion (Montgomery's trick)
  std::vector<G2Jac> jac(32 * 256);
  G2Jac base = g2_jac_from_affine(g2_generator());
  for (int j = 0; j < 32; j++) {
    jac[j * 256] = G2Jac::identity();
    G2Jac cur = base;
    for (int d = 1; d < 256; d++) {
      jac[j * 256 + d] = cur;
      cur = g2_jac_add(cur, base);
    }
    for (int k = 0; k < 8; k++) base = g2_jac_dbl(base);
  }
  std::vector<G2Affine> aff(jac.size());
  std::vector<Fq2> pref(jac.size());
  Fq2 acc = Fq2::one();
  for (size_t i = 0; i < jac.size(); i++) {
    pref[i] = acc;
    if (!jac[i].is_identity()) acc = acc * jac[i].z;
  }
  acc = acc.inv();
  for (size_t i = jac.size(); i-- > 0;) {
    if (jac[i].is_identity()) {
      aff[i] = G2Affine::identity();
      continue;
    }
    const Fq2 zi = pref[i] * acc;
    acc = acc * jac[i].z;
    const Fq2 zi2 = zi.sqr();
    aff[i] = {jac[i].x * zi2, jac[i].y * zi2 * zi};
  }
  G2Affine* table = nullptr;
  CQ_HIP(c, hipMalloc(&table, aff.size() * sizeof(G2Affine)));
  hipError_t e = hipMemcpyAsync(table, aff.data(), aff.size() * sizeof(G2Affine), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    g2_fixed_base_powers_kernel<<<(count + G2_THREADS - 1) / G2_THREADS, G2_THREADS, 0, c->stream>>>(s, count, table, out_dev);
    e = hipGetLastError();
  }
  hipStreamSynchronize(c->stream);
  hipFree(table);
  return e == hipSuccess ? CQ_OK : c->hip_fail(e, "g2 srs powers");
}

}  // namespace cq

// G1 MSM engine, steps 4 and 5 of the pipeline (msm.hip has the overview): the accumulate kernel, the combine levels, the
// bucket reduction (row / column sums, weighted sums, their quad forms) or -- bucket-sum launches -- the buckets as affine
// points, and the kernels that build the window tables.  The host functions enqueue a stage on the buffers of an MsmBuffers view.
#include <algorithm>
#include <cstdlib>
#include "msm.hpp"
#include "curve29.hpp"
#include "ctx.hpp"

namespace cq {

// ---- 4. bucket accumulation ----------------------------------------------------------------
// largest g in [0,B) with off[g] <= j   (off is non-decreasing, off[0] = 0, j < off[B])
static __device__ __forceinline__ uint32_t owner_of(const uint32_t* __restrict__ off, uint32_t B, uint32_t j) {
  uint32_t lo = 0, hi = B;  // invariant: off[lo] <= j < off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off[mid] <= j) lo = mid; else hi = mid;
  }
  return lo;
}

// Who sums a list of MSM_SHORT_MIN < t <= MSM_SHORT partial sums?  A lane group walks it serially (t / Q dependent
// additions, work-optimal), a wave sums it as a tree (one load per lane and six shuffle levels: ~8x the lane-operations,
// a third of the depth).  With hundreds of thousands of such lists the launch is throughput-bound and the lane groups
// win; with a few (a sparse or skewed column: the SHA limb columns, the multiplicities m) the launch is waiting for its
// longest dependent chain and the waves win.  Decided on the device from the number of wave slots of the level
// (`slots` = off_cur[Bt], already there from the plan scan), the same way by both halves of the kernel.
static __device__ __forceinline__ uint32_t combine_short_limit(uint32_t slots) {
  return slots <= MSM_WAVE_BUDGET ? MSM_SHORT_MIN : MSM_SHORT;
}

// level 1: lane j owns sub-list j of <= MSM_S1 point indices
__global__ __launch_bounds__(MSM_ACC_THREADS) void msm_accumulate_kernel(
    const G1Affine* const* __restrict__ bases, uint32_t buckets_per_msm, uint32_t pre,
    const uint64_t* __restrict__ table_strides, const uint64_t* __restrict__ list_src, const uint32_t* __restrict__ sorted,
    const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off0,
    const uint32_t* __restrict__ t1, const uint32_t* __restrict__ off1, uint32_t Bt, XYZZ* __restrict__ partial,
    XYZZ* __restrict__ buckets) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= off1[Bt]) return;
  const uint32_t g = owner_of(off1, Bt, j);
  const uint32_t msm = g / buckets_per_msm;
  const G1Affine* __restrict__ pts = bases[msm];
  const size_t table_stride = pre ? (size_t)table_strides[msm] : 0;
  const uint32_t r = j - off1[g];
  // the bucket's cnt entries are cut into t = ceil(cnt / s1) sub-lists of EQUAL length (+-1): a wave runs as
  // long as its longest lane, so 40 entries are better served as 20 + 20 than as 32 + 8
  // an MSM over the same scalars as an earlier one of the launch (b0 and p of a CQ lookup) reads that one's lists
  const uint32_t list0 = off0[(uint32_t)list_src[msm] * buckets_per_msm + (g - msm * buckets_per_msm)];
  const uint32_t t = t1[g], n_g = cnt[g];
  const uint32_t lo = list0 + (uint32_t)(((uint64_t)n_g * r) / t);
  const uint32_t hi = list0 + (uint32_t)(((uint64_t)n_g * (r + 1)) / t);
  XYZZ29 acc = XYZZ29::identity();
  // Software pipeline: the table point of entry e+1 (a dependent, essentially random 64-byte gather) and the
  // index of entry e+2 are requested before the ~10 products of entry e are computed.
  // precomputed mode: table[w][i] = 2^(c*w) * base[i], stored in the kernels' R' limb form; otherwise the
  // caller's array of R = 2^256 values is converted on the fly
  auto addr_of = [&](uint32_t ix) {
    return pre ? (size_t)((ix >> 26) & 31u) * table_stride + (ix & 0x03ffffffu) : (size_t)(ix & 0x7fffffffu);
  };
  uint32_t ix_cur = lo < hi ? sorted[lo] : 0u;
  uint32_t ix_next = lo + 1 < hi ? sorted[lo + 1] : 0u;
  uint32_t wx[8], wy[8];
  if (lo < hi) {
    const G1Affine* q = pts + addr_of(ix_cur);
    ld8(&q->x, wx);
    ld8(&q->y, wy);
  }
  for (uint32_t e = lo; e < hi; e++) {
    Affine29 p;
    p.x = Fq29::unpack(wx);
    p.y = Fq29::unpack(wy);
    const uint32_t neg = ix_cur >> 31;
    ix_cur = ix_next;
    if (e + 1 < hi) {
      const G1Affine* q = pts + addr_of(ix_cur);
      ld8(&q->x, wx);
      ld8(&q->y, wy);
    }
    ix_next = e + 2 < hi ? sorted[e + 2] : 0u;
    if (!pre) {  // R = 2^256 values of a caller's array
      Fq29 f;
      CQ_UNROLL for (int i = 0; i < 9; i++) f.a[i] = CONSTS29<FqP>.from256[i];
      p.x = Fq29::mul(p.x, f);
      p.y = Fq29::mul(p.y, f);
    }
    if (neg && !p.is_identity()) p.y = Fq29::neg<2>(p.y);
    xyzz29_add_affine(acc, p);
  }
  store_xyzz29(t == 1 ? buckets + g : partial + j, acc);
}

// Level k >= 2 in ONE launch.  Blocks [0, short_blocks): Q lanes per BUCKET sum the short lists (2..limit partial sums
// of level k-1, always the whole bucket): indexed by bucket, no search, a bucket that is empty, already final (one
// partial sum) or long costs one load; a group sums strided parts and folds them with log2(Q) shuffles.  The remaining
// blocks: one WAVE per sub-list of <= MSM_S2 partial sums of the longer lists (strided lane sums + 6-step shuffle tree);
// only those lists own slots at level k, so off_cur[Bt] is small (usually zero) and almost every wave leaves at the
// first test.  The two halves write different buckets and do not depend on each other: one launch instead of two
// keeps the level's latency at the longer of the two chains.
template <uint32_t Q>
__global__ __launch_bounds__(256, 3) void msm_combine_level_kernel(
    const XYZZ* __restrict__ prev, const uint32_t* __restrict__ t_prev, const uint32_t* __restrict__ off_prev,
    const uint32_t* __restrict__ t_cur, const uint32_t* __restrict__ off_cur, uint32_t Bt, uint32_t short_blocks,
    XYZZ* __restrict__ partial, XYZZ* __restrict__ buckets) {
  CQ_CRITICAL_WAVES();
  const uint32_t slots = off_cur[Bt];
  const uint32_t limit = combine_short_limit(slots);
  if (blockIdx.x < short_blocks) {
    const uint32_t gt = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t g = gt / Q, sub = gt % Q;
    const uint32_t tp = g < Bt ? t_prev[g] : 0;
    const bool mine = tp >= 2 && tp <= limit;
    if (!__any(mine)) return;  // wave-uniform
    const uint32_t lo = mine ? off_prev[g] : 0;
    XYZZ29 acc = XYZZ29::identity();
    if (mine && sub < tp) {  // the next partial sum is on its way while the current one is added
      XYZZRaw nxt = load_xyzz_raw(prev + lo + sub);
      for (uint32_t e = sub; e < tp; e += Q) {
        const XYZZ29 cur = unpack_xyzz29(nxt);
        if (e + Q < tp) nxt = load_xyzz_raw(prev + lo + e + Q);
        xyzz29_add(acc, cur);
      }
    }
    xyzz29_tree_sum<Q>(acc, sub, mine);
    if (mine && sub == 0) store_xyzz29(buckets + g, acc);
    return;
  }
  // (The slots are few -- usually none -- but their BOUND, which is all the host knows, is in the millions at k >= 20: the
  // wave half is a capped number of blocks that stride over the slots, not one block per four possible slots; the empty
  // blocks alone were ~0.3 ms of a k = 20 proof and ~1 ms at k = 22.)
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t nwaves = (gridDim.x - short_blocks) * (blockDim.x >> 6);
#pragma unroll 1
  // (j through readfirstlane: wave-uniform, and everything derived from it -- the owner search, the list bounds -- stays in
  // scalar registers; as a vector value the loop took the kernel over the 168 registers of its three waves per SIMD, into scratch)
  for (uint32_t j = __builtin_amdgcn_readfirstlane((blockIdx.x - short_blocks) * (blockDim.x >> 6) + (threadIdx.x >> 6)); j < slots; j += nwaves) {
  const uint32_t g = owner_of(off_cur, Bt, j);
  const uint32_t tp = t_prev[g];
  if (tp <= limit) continue;  // a lane group of the other half owns this list (throughput-bound launch)
  const uint32_t r = j - off_cur[g];
  const uint32_t lo = off_prev[g] + r * MSM_S2;
  const uint32_t hi = min(off_prev[g] + tp, lo + MSM_S2);
  // Four lanes per addition (quad_add, curve29.hpp): this half only runs for the few long lists of a launch, which the
  // launch then waits for.  Quad q sums the partial sums lo + q, lo + q + 16, .. (lane r of the quad their coordinate r),
  // an XOR butterfly over the quads that hold data folds them: <= 4 + 4 additions of ~2.4 us instead of 1 + 6 of ~5 us.
  const uint32_t role = lane & 3u, quad = lane >> 2, len = hi - lo;
  Fq29 F = Fq29::zero();
  if (quad < len) F = quad_load(prev + lo + quad, role);
#pragma unroll 1
  for (uint32_t e = quad + 16; e < ((len + 15u) & ~15u); e += 16) {  // (the same trip count for every quad: the permutes need all lanes)
    Fq29 G = Fq29::zero();
    if (e < len) G = quad_load(prev + lo + e, role);
    F = quad_add(F, G);
  }
  const uint32_t nq = len < 16 ? len : 16;  // quads holding data
  F = quad_wave_sum(F, nq > 8 ? 32 : nq > 4 ? 16 : nq > 2 ? 8 : nq > 1 ? 4 : 0);
  quad_store(t_cur[g] == 1 ? buckets + g : partial + j, F);
  }
}

// ---- precomputed window tables (one-off setup) -----------------------------------------------------------
// Tables are library-internal, so they hold the accumulate kernel's own representation: coordinates in
// Montgomery form with R' = 2^261, packed into 8 x u32 (field29.hpp).  Window 0 = the caller's points converted.
static __device__ __forceinline__ void store_affine29(G1Affine* dst, const Affine29& p) {
  uint32_t w[8];
  p.x.pack(w);
  st8(&dst->x, w);
  p.y.pack(w);
  st8(&dst->y, w);
}
__global__ __launch_bounds__(256) void msm_table0_kernel(const G1Affine* __restrict__ bases, G1Affine* __restrict__ table, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  store_affine29(table + i, load_affine29(bases + i, true));
}
// next[i] = 2^c * prev[i] (affine in, affine out): the doublings and the inversion run on the canonical field type
__global__ __launch_bounds__(256) void msm_pre_kernel(const G1Affine* __restrict__ prev, G1Affine* __restrict__ next, uint32_t n,
                                                      uint32_t c) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Affine29 p29 = load_affine29(prev + i, false);
  const G1Affine p = {p29.x.to_mont256(), p29.y.to_mont256()};
  XYZZ a = xyzz_dbl_affine(p);
  for (uint32_t k = 1; k < c; k++) a = xyzz_dbl(a);
  G1Affine r = G1Affine::identity();
  if (!a.is_identity()) {
    const Fq iv = (a.zz * a.zzz).inv();
    r.x = a.x * (iv * a.zzz);
    r.y = a.y * (iv * a.zz);
  }
  store_affine29(next + i, {Fq29::from_mont256(r.x), Fq29::from_mont256(r.y)});
}

int msm_precompute_tables(cq_ctx* ctx, const G1Affine* bases, uint32_t n, uint32_t c, G1Affine* table /* W*n */) {
  const uint32_t W = (255 + c - 1) / c;
  hipStream_t s = ctx->stream;
  msm_table0_kernel<<<(n + 255) / 256, 256, 0, s>>>(bases, table, n);
  for (uint32_t w = 1; w < W; w++)
    msm_pre_kernel<<<(n + 255) / 256, 256, 0, s>>>(table + (size_t)(w - 1) * n, table + (size_t)w * n, n, c);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// (no __restrict__: out may be bases -- every lane loads its point before it stores it)
__global__ __launch_bounds__(256) void msm_bases29_kernel(const G1Affine* bases, G1Affine* out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Affine29 p = load_affine29(bases + i, true);
  store_affine29(out + i, p);
}
int msm_bases29(cq_ctx* ctx, const G1Affine* bases, uint32_t n, G1Affine* out) {
  msm_bases29_kernel<<<(n + 255) / 256, 256, 0, ctx->stream>>>(bases, out, n);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- bucket-sum launches (msm_bucket_sums): the first `count` buckets of every MSM as affine points ------------------
// A launch that is given the bucket j(i) of every point i (the index front) has one entry per point at most, in window 0, and
// bucket j ends up holding sum_{i : j(i) = j} base[i]: the launch stops there and hands the bucket sums out in the callers'
// R = 2^256 affine layout (one inversion per bucket, all independent), ready to be the bases of a later MSM.  A bucket
// without entries was never written (msm_rowcol_kernel) and stands for the identity.
__global__ __launch_bounds__(256) void msm_buckets_affine_kernel(const XYZZ* __restrict__ buckets, const uint32_t* __restrict__ t1, uint32_t B,
                                                                 uint32_t count, G1Affine* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, m = blockIdx.y;
  if (i >= count) return;
  const size_t g = (size_t)m * B + i;
  G1Affine r = G1Affine::identity();
  if (t1[g]) {
    const XYZZ29 v = load_xyzz29(buckets + g);
    if (!v.is_identity()) {
      const Fq x = v.x.reduced().to_mont256(), y = v.y.to_mont256(), zz = v.zz.to_mont256(), zzz = v.zzz.to_mont256();
      const Fq iv = (zz * zzz).inv();
      r.x = x * (iv * zzz);
      r.y = y * (iv * zz);
    }
  }
  G1Affine* o = out + (size_t)m * count + i;
  uint32_t w[8];
  for (int k = 0; k < 8; k++) w[k] = r.x.v.l[k];
  st8(&o->x, w);
  for (int k = 0; k < 8; k++) w[k] = r.y.v.l[k];
  st8(&o->y, w);
}

// ---- 5. reduction: sum_{b=1..M} b * B_b per bucket set ---------------------------------------------------
// Every dependent EC addition costs a lone wave ~9 us whatever the number of busy lanes, so the reduction is shaped
// for depth, not work.  Buckets are read as a rows x cols matrix (b = cols * hi + lo + 1, cols = min(M, 128)):
//     sum_b b B_b  =  cols * sum_hi hi R_hi  +  sum_lo (lo + 1) C_lo,     R = row sums, C = column sums.
// Kernel 1: 16 or 32 lanes per row / column sum (a few buckets per lane serially, then a shuffle tree), all lines
// independent.  Kernel 2: per bucket set two waves, one per weighted sum of <= 128 terms
// (pair sums, suffix scan by shuffles, one tree); the host applies "cols *" and joins the two.  ~11 + ~16 dependent
// operations instead of the ~46 of a lane-serial running sum over 1024-bucket groups.
// A wave serves 64 / SEG rows (or columns): SEG lanes per line, each summing cols / SEG consecutive buckets of it
// serially, then a log2(SEG)-level shuffle tree.  SEG = 16 (depth 8 + 4, every lane busy in the serial part) when a
// launch has many bucket sets -- with one wave per line and a 6-level tree only a quarter of the lane-operations were
// useful and the kernel was VALU-throughput bound at batch 16; SEG = 32 for a middling number of sets.  Launches of a few
// sets, which are latency-bound and leave most SIMDs idle anyway, take msm_rowcol_quad_kernel instead.
template <uint32_t SEG>
__global__ __launch_bounds__(64) void msm_rowcol_kernel(const XYZZ* __restrict__ buckets, const uint32_t* __restrict__ t1, uint32_t M,
                                                        uint32_t rows, uint32_t cols, XYZZ* __restrict__ sums /*[sets][rows + cols]*/) {
  CQ_CRITICAL_WAVES();
  constexpr uint32_t LINES = 64 / SEG;
  const uint32_t set = blockIdx.y, lane = threadIdx.x;
  const uint32_t q = blockIdx.x * LINES + lane / SEG, seg = lane % SEG;  // line: row q or column q - rows
  const XYZZ* Bk = buckets + (size_t)set * M;
  // a bucket without entries (no level-1 sub-list) was never written -- the workspace's buckets are not cleared, 128 bytes
  // each: 180 MB per round-2 launch at k >= 20 -- and stands for the identity
  const uint32_t* Tk = t1 + (size_t)set * M;
  XYZZ29 acc = XYZZ29::identity();
  if (q < rows) {  // R_q = sum_lo B[q][lo]
    const uint32_t per = (cols + SEG - 1) / SEG;
    for (uint32_t lo = seg * per; lo < min(cols, (seg + 1) * per); lo++)
      if (Tk[(size_t)q * cols + lo]) xyzz29_add(acc, load_xyzz29(Bk + (size_t)q * cols + lo));
  } else if (q < rows + cols) {  // C_lo = sum_hi B[hi][lo]
    const uint32_t lo = q - rows, per = (rows + SEG - 1) / SEG;
    for (uint32_t hi = seg * per; hi < min(rows, (seg + 1) * per); hi++)
      if (Tk[(size_t)hi * cols + lo]) xyzz29_add(acc, load_xyzz29(Bk + (size_t)hi * cols + lo));
  }
  xyzz29_tree_sum<SEG>(acc, seg);
  if (seg == 0 && q < rows + cols) store_xyzz29(sums + (size_t)set * (rows + cols) + q, acc);
}

// sum_{j < count} (j + first_weight) X_j, count <= 128, as sum_t 2^t S_t with S_t = the sum of the X_j whose index has
// bit t set: seven independent 64-term trees (six shuffle levels) instead of a suffix scan followed by a tree (fifteen
// dependent additions, ~190 us for a lone wave -- the longest single stretch of a launch's tail; a doubling costs a
// lone wave as much as an addition, so the "2^t" may not run here either).  The kernel stops at the S_t: the Horner
// over t, the plain total of the "+ first_weight" term, the log2(cols) doublings and the last additions are ~33 group
// operations per bucket set for the host (msm_set_value), which needs a fraction of a microsecond for each where a
// lone wave needs ~10 us.  out[set][0..6] = row planes, [7..13] = column planes, [14] = column total (MSM_SET_POINTS).
// One WAVE per block (and so, with a few dozen blocks on 256 CUs, per SIMD): two waves of such a chain on one SIMD share
// its issue slots and each runs at half speed -- eight-wave blocks made this kernel take 150-220 us for six levels.
__global__ __launch_bounds__(64) void msm_weighted_kernel(const XYZZ* __restrict__ sums, uint32_t rows, uint32_t cols,
                                                          G1Jac* __restrict__ out) {
  CQ_CRITICAL_WAVES();
  const uint32_t set = blockIdx.x / MSM_SET_POINTS, plane = blockIdx.x % MSM_SET_POINTS, lane = threadIdx.x;
  const uint32_t which = plane >= 7 ? 1u : 0u;
  const XYZZ* X = sums + (size_t)set * (rows + cols) + (which ? rows : 0);
  const uint32_t count = which ? cols : rows;
  XYZZ29 v = XYZZ29::identity();
  if (plane < 14) {
    const uint32_t t = plane - 7 * which;
    const uint32_t j = ((lane >> t) << (t + 1)) | (1u << t) | (lane & ((1u << t) - 1u));  // lane-th index with bit t set
    if (j < count) v = load_xyzz29(X + j);
  } else {
    if (lane < count) v = load_xyzz29(X + lane);
    if (lane + 64 < count) xyzz29_add(v, load_xyzz29(X + lane + 64));
  }
  xyzz29_tree_sum<64>(v, lane);
  if (lane == 0) out[(size_t)set * MSM_SET_POINTS + plane] = xyzz29_to_jac(v);
}

// Row / column sums with FOUR lanes per addition (quad_add), for launches of a few bucket sets: one 256-thread block per
// line of <= 128 buckets -- quad q takes buckets q and q + 64 of the line (lane r of the quad their coordinate r), then the
// same butterfly as msm_weighted_quad_kernel: seven additions of ~2.4 us deep instead of 2 + 6 of ~5 us.
__global__ __launch_bounds__(256) void msm_rowcol_quad_kernel(const XYZZ* __restrict__ buckets, const uint32_t* __restrict__ t1, uint32_t M,
                                                              uint32_t rows, uint32_t cols, XYZZ* __restrict__ sums /*[sets][rows + cols]*/) {
  CQ_CRITICAL_WAVES();
  __shared__ uint32_t xs[4][4][9];
  const uint32_t set = blockIdx.y, q = blockIdx.x;  // line: row q or column q - rows
  const uint32_t wave = threadIdx.x >> 6, role = threadIdx.x & 3u, quad = threadIdx.x >> 2;
  const XYZZ* Bk = buckets + (size_t)set * M;
  const uint32_t* Tk = t1 + (size_t)set * M;
  const bool is_row = q < rows;
  const uint32_t len = is_row ? cols : rows;
  auto load_coord = [&](uint32_t e) {  // coordinate `role` of the line's e-th bucket; identity for a bucket without entries
    Fq29 r = Fq29::zero();
    if (e < len) {
      const size_t idx = is_row ? (size_t)q * cols + e : (size_t)e * cols + (q - rows);
      if (Tk[idx]) r = quad_load(Bk + idx, role);
    }
    return r;
  };
  const Fq29 F0 = load_coord(quad), G0 = load_coord(quad + 64);
  const Fq29 F = quad_block_sum(quad_add(F0, G0), xs);
  if (wave != 0) return;
  quad_store(sums + (size_t)set * (rows + cols) + q, F);
}

// The same bit-plane sums with FOUR lanes per addition (quad_add, curve29.hpp), for launches of a few bucket sets -- the
// plain kernel's six tree levels are six dependent general additions of ~5 us each on a lone wave; a quad needs ~2.4.
// 256 threads = 64 quads per plane: quad q takes the plane's q-th term (lane r of the quad its coordinate r), an XOR
// butterfly over the 16 quads of a wave (4 levels, every quad ends with the wave's sum), the four waves' sums through
// LDS, two more levels in wave 0.  Results are the same group elements as msm_weighted_kernel's (sums in another order).
__global__ __launch_bounds__(256) void msm_weighted_quad_kernel(const XYZZ* __restrict__ sums, uint32_t rows, uint32_t cols,
                                                                G1Jac* __restrict__ out) {
  CQ_CRITICAL_WAVES();
  __shared__ uint32_t xs[4][4][9];
  const uint32_t set = blockIdx.x / MSM_SET_POINTS, plane = blockIdx.x % MSM_SET_POINTS;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, role = threadIdx.x & 3u, quad = threadIdx.x >> 2;
  const uint32_t which = plane >= 7 ? 1u : 0u;
  const XYZZ* X = sums + (size_t)set * (rows + cols) + (which ? rows : 0);
  const uint32_t count = which ? cols : rows;
  Fq29 F = Fq29::zero();
  if (plane < 14) {
    const uint32_t t = plane - 7 * which;
    const uint32_t j = ((quad >> t) << (t + 1)) | (1u << t) | (quad & ((1u << t) - 1u));  // quad-th index with bit t set
    if (j < count) F = quad_load(X + j, role);
  } else {
    if (quad < count) F = quad_load(X + quad, role);
    Fq29 G = Fq29::zero();
    if (quad + 64 < count) G = quad_load(X + quad + 64, role);
    F = quad_add(F, G);
  }
  F = quad_block_sum(F, xs);
  if (wave != 0) return;
  const XYZZ29 v = quad_to_xyzz29(F);
  if (lane == 0) out[(size_t)set * MSM_SET_POINTS + plane] = xyzz29_to_jac(v);
}

// ---- host: the stages of a launch's middle and tail ------------------------------------------------------------
void msm_accumulate(hipStream_t s, const MsmLayout& L, const MsmBuffers& b) {
  const uint32_t Bt = L.Bt;
  msm_accumulate_kernel<<<(uint32_t)((L.tmax[0] + MSM_ACC_THREADS - 1) / MSM_ACC_THREADS), MSM_ACC_THREADS, 0, s>>>(
      b.bases, L.B, L.pre ? 1u : 0u, b.strides, b.src, b.sorted, b.counts, b.off, b.tk, b.off + (size_t)(Bt + 1), Bt, b.part[0], b.buckets);
}

void msm_combine_levels(hipStream_t s, const MsmLayout& L, const MsmBuffers& b) {
  const uint32_t Bt = L.Bt;
  for (uint32_t k = 1; k < L.levels; k++) {
    const uint32_t* t_prev = b.tk + (size_t)(k - 1) * Bt;
    const uint32_t* off_prev = b.off + (size_t)k * (Bt + 1);
    const uint32_t* t_cur = b.tk + (size_t)k * Bt;
    const uint32_t* off_cur = b.off + (size_t)(k + 1) * (Bt + 1);
    // ping-pong: level k+1 reads part[(k-1)&1], writes part[k&1]
    const uint32_t q = Bt <= (1u << 18) ? 4u : Bt <= (1u << 19) ? 2u : 1u;  // lanes per bucket, see the kernel
    const uint32_t cs_blocks = (uint32_t)(((uint64_t)Bt * q + 255) / 256);
    // (CQ_MSM_COMBINE_WAVE_BLOCKS: tests shrink the cap so that small launches stride too)
    static const uint32_t wave_cap = getenv("CQ_MSM_COMBINE_WAVE_BLOCKS") ? (uint32_t)std::max(1, atoi(getenv("CQ_MSM_COMBINE_WAVE_BLOCKS"))) : MSM_COMBINE_WAVE_BLOCKS;
    const uint32_t wv_blocks = (uint32_t)std::min<uint64_t>((L.tmax[k] + 3) / 4, wave_cap);
    auto combine = [&](auto kernel) {
      kernel<<<cs_blocks + wv_blocks, 256, 0, s>>>(b.part[(k - 1) & 1], t_prev, off_prev, t_cur, off_cur, Bt, cs_blocks, b.part[k & 1], b.buckets);
    };
    if (q == 4) combine(msm_combine_level_kernel<4>);
    else if (q == 2) combine(msm_combine_level_kernel<2>);
    else combine(msm_combine_level_kernel<1>);
  }
}

void msm_emit_buckets(hipStream_t s, const MsmLayout& L, const MsmBuffers& b, uint32_t count, G1Affine* out) {
  msm_buckets_affine_kernel<<<dim3((count + 255) / 256, L.batch), 256, 0, s>>>(b.buckets, b.tk, L.B, count, out);
}

void msm_reduce_sets(hipStream_t s, const MsmLayout& L, const MsmBuffers& b, G1Jac* window_sums) {
  const uint32_t sets = L.batch * L.Wb;
  // (few sets: the launch waits for chains of dependent additions, and four lanes per addition shorten them; many sets: the
  // SIMDs are busy, and one lane per addition is half the instructions.)
  constexpr uint32_t QUAD_ROWCOL_SETS = 4, SEG32_SETS = 12;
  if (sets <= QUAD_ROWCOL_SETS)
    msm_rowcol_quad_kernel<<<dim3(L.rows + L.cols, sets), 256, 0, s>>>(b.buckets, b.tk, L.M, L.rows, L.cols, b.pairs);
  else if (sets <= SEG32_SETS)
    msm_rowcol_kernel<32><<<dim3((L.rows + L.cols + 1) / 2, sets), 64, 0, s>>>(b.buckets, b.tk, L.M, L.rows, L.cols, b.pairs);
  else
    msm_rowcol_kernel<16><<<dim3((L.rows + L.cols + 3) / 4, sets), 64, 0, s>>>(b.buckets, b.tk, L.M, L.rows, L.cols, b.pairs);
  // (measured at k = 18: 21 sets -- 1 260 four-wave blocks -- 88 -> 54 us; from ~2 waves per SIMD on the plain kernel's
  // half-as-many instructions win)
  constexpr uint32_t QUAD_WEIGHTED_WAVES = 2048;
  if (sets * MSM_SET_POINTS * 4 <= QUAD_WEIGHTED_WAVES) msm_weighted_quad_kernel<<<MSM_SET_POINTS * sets, 256, 0, s>>>(b.pairs, L.rows, L.cols, window_sums);
  else msm_weighted_kernel<<<MSM_SET_POINTS * sets, 64, 0, s>>>(b.pairs, L.rows, L.cols, window_sums);
}

}  // namespace cq

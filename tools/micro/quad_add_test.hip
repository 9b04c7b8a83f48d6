// quad_add (curve29.hpp: one general addition by four lanes) against xyzz29_add on one wave, every special case, and the
// sums built on it and on xyzz29_add (quad_wave_sum, quad_block_sum, quad_store, xyzz29_tree_sum) against a lane-serial chain:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -I sha2_on_cq_halo2_amd/csrc tools/micro/quad_add_test.hip -o /tmp/qt && /tmp/qt
// (tests/test_msm_gpu.py::test_quad_add_matches_lane_serial_addition builds and runs it on the GPU box)
#include <hip/hip_runtime.h>
#include <cstdio>
#include "curve29.hpp"
using namespace cq;

// mode 0: general; odd quads: 1 P2 = identity, 2 P1 = identity, 3 P2 = P1 (doubling), 4 P2 = -P1 (cancellation), 5 both identity
__global__ __launch_bounds__(64) void test(uint32_t* out, uint32_t mode) {
  const uint32_t lane = threadIdx.x, quad = lane >> 2, role = lane & 3;
  Affine29 g;  // the generator (1, 2) in R' form
  g.x = Fq29::one();
  g.y = Fq29::one() + Fq29::one();
  g.y.normalise();
  auto mulk = [&](uint32_t k) {
    XYZZ29 a = XYZZ29::identity();
    for (uint32_t i = 0; i < k; i++) xyzz29_add_affine(a, g);
    return a;
  };
  XYZZ29 p1 = mulk(2 + quad), p2 = mulk(40 + 3 * quad);
  if (quad & 1) {
    if (mode == 1 || mode == 5) p2 = XYZZ29::identity();
    if (mode == 2 || mode == 5) p1 = XYZZ29::identity();
    if (mode == 3) p2 = mulk(2 + quad);  // the same point (and the same coordinates)
    if (mode == 4) {
      p2 = p1;
      p2.y = Fq29::neg<4>(p2.y);
    }
  }
  XYZZ29 ref = p1;
  xyzz29_add(ref, p2);
  const Fq29 F = role == 0 ? p1.x : role == 1 ? p1.y : role == 2 ? p1.zz : p1.zzz;
  const Fq29 G = role == 0 ? p2.x : role == 1 ? p2.y : role == 2 ? p2.zz : p2.zzz;
  const Fq29 R = quad_add(F, G);
  const XYZZ29 q = quad_to_xyzz29(R);
  // the same affine point?  x_ref zz_q == x_q zz_ref and y_ref zzz_q == y_q zzz_ref, and identity <=> identity
  const Fq a = (ref.x * q.zz).to_mont256(), b = (q.x * ref.zz).to_mont256();
  const Fq c = (ref.y * q.zzz).to_mont256(), d = (q.y * ref.zzz).to_mont256();
  out[lane] = (a == b) && (c == d) && (ref.is_identity() == q.is_identity());
}
// ---- the sums of the launch tails against a lane-serial xyzz29_add chain over the same n <= 128 terms ----------------
// One 256-thread block.  Term i is k_i G (k_i distinct); mix 1: every third term the identity; mix 2: all terms the same
// point (a doubling at every tree level); mix 3: terms 2 j and 2 j + 1 opposite (cancellations).  Every result goes to a
// slot of `res` in packed form and is compared with the chain's after both are normalised to affine.
constexpr uint32_t SUM_TERMS = 128, SLOT_WAVE = 0, SLOT_WAVE_STORE = 64, SLOT_BLOCK_STORE = 68, SLOT_BLOCK = 69, SLOT_TREE = 73,
                   SUM_SLOTS = SLOT_TREE + 5 * 128;
static __host__ __device__ uint32_t butterfly_from(uint32_t nq) { return nq > 8 ? 32 : nq > 4 ? 16 : nq > 2 ? 8 : nq > 1 ? 4 : 0; }
static __host__ __device__ bool tree_group_live(uint32_t width, uint32_t group) { return width == 64 || group % 3 != 2; }

static __device__ __forceinline__ bool same_affine_point(const XYZZ29& a, const XYZZ29& b) {
  Fq ax[2], ay[2];
  bool inf[2];
#pragma unroll 1
  for (int i = 0; i < 2; i++) {
    const XYZZ29& v = i ? b : a;
    inf[i] = v.is_identity();
    ax[i] = ay[i] = Fq::zero();
    if (!inf[i]) {
      const Fq zz = v.zz.to_mont256(), zzz = v.zzz.to_mont256(), iv = (zz * zzz).inv();
      ax[i] = v.x.reduced().to_mont256() * (iv * zzz);
      ay[i] = v.y.to_mont256() * (iv * zz);
    }
  }
  return inf[0] == inf[1] && ax[0] == ax[1] && ay[0] == ay[1];
}

template <uint32_t WIDTH>
static __device__ __forceinline__ void tree_case(const XYZZ* pts, uint32_t n, XYZZ* res, uint32_t* valid, uint32_t slot0) {
  const uint32_t pos = threadIdx.x % WIDTH, group = threadIdx.x / WIDTH;
  const bool live = tree_group_live(WIDTH, group);  // (the other groups only take part in the shuffles)
  XYZZ29 acc = XYZZ29::identity();
#pragma unroll 1
  for (uint32_t e = pos; e < n; e += WIDTH) xyzz29_add(acc, load_xyzz29(pts + e));
  xyzz29_tree_sum<WIDTH>(acc, pos, live);
  if (live && pos == 0) {
    store_xyzz29(res + slot0 + group, acc);
    valid[slot0 + group] = 1;
  }
}

__global__ __launch_bounds__(256) void sums(XYZZ* pts, XYZZ* res, uint32_t* valid, uint32_t* out, uint32_t n, uint32_t mix) {
  __shared__ uint32_t xs[4][4][9];
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6, role = t & 3u;
  if (t < n) {
    const uint32_t j = mix == 3 ? t >> 1 : t;
    const uint32_t k = mix == 2 ? 5u : 1u + (37u * j + 11u) % 251u;
    Affine29 g;
    g.x = Fq29::one();
    g.y = Fq29::one() + Fq29::one();
    g.y.normalise();
    XYZZ29 a = XYZZ29::identity();
#pragma unroll 1
    for (uint32_t i = 0; i < k; i++) xyzz29_add_affine(a, g);
    if (mix == 1 && t % 3 == 1) a = XYZZ29::identity();
    if (mix == 3 && (t & 1u)) a.y = Fq29::neg<4>(a.y);
    store_xyzz29(pts + t, a);
  }
  __threadfence();
  __syncthreads();
  XYZZ29 ref = XYZZ29::identity();
#pragma unroll 1
  for (uint32_t e = 0; e < n; e++) xyzz29_add(ref, load_xyzz29(pts + e));

  {  // quad_wave_sum as the combine kernel's wave half uses it: quad q of every wave sums the terms q, q + 16, ..
    const uint32_t quad = lane >> 2;
    Fq29 F = Fq29::zero();
    if (quad < n) F = quad_load(pts + quad, role);
#pragma unroll 1
    for (uint32_t e = quad + 16; e < ((n + 15u) & ~15u); e += 16) {
      Fq29 G = Fq29::zero();
      if (e < n) G = quad_load(pts + e, role);
      F = quad_add(F, G);
    }
    const uint32_t from_d = butterfly_from(n < 16 ? n : 16);
    F = quad_wave_sum(F, (int)from_d);
    const XYZZ29 v = quad_to_xyzz29(F);
    if (role == 0 && quad < (from_d ? from_d / 2 : 1u)) {  // every quad of the butterfly ends with the sum
      store_xyzz29(res + SLOT_WAVE + 16 * wave + quad, v);
      valid[SLOT_WAVE + 16 * wave + quad] = 1;
    }
    quad_store(res + SLOT_WAVE_STORE + wave, F);
    if (lane == 0) valid[SLOT_WAVE_STORE + wave] = 1;
  }
  {  // quad_block_sum as the quad tail kernels use it: quad q of the block takes the terms q and q + 64
    const uint32_t quad = t >> 2;
    Fq29 F0 = Fq29::zero(), G0 = Fq29::zero();
    if (quad < n) F0 = quad_load(pts + quad, role);
    if (quad + 64 < n) G0 = quad_load(pts + quad + 64, role);
    const Fq29 F = quad_block_sum(quad_add(F0, G0), xs);
    const XYZZ29 v = quad_to_xyzz29(F);
    if (wave == 0) {
      quad_store(res + SLOT_BLOCK_STORE, F);
      if (role == 0 && quad < 4) {
        store_xyzz29(res + SLOT_BLOCK + quad, v);
        valid[SLOT_BLOCK + quad] = 1;
      }
      if (lane == 0) valid[SLOT_BLOCK_STORE] = 1;
    }
  }
  tree_case<2>(pts, n, res, valid, SLOT_TREE);
  tree_case<4>(pts, n, res, valid, SLOT_TREE + 128);
  tree_case<16>(pts, n, res, valid, SLOT_TREE + 256);
  tree_case<32>(pts, n, res, valid, SLOT_TREE + 384);
  tree_case<64>(pts, n, res, valid, SLOT_TREE + 512);
  __threadfence();
  __syncthreads();
#pragma unroll 1
  for (uint32_t s = t; s < SUM_SLOTS; s += 256)
    if (valid[s]) out[s] = same_affine_point(load_xyzz29(res + s), ref) ? 1u : 2u;
}

static int run_sums() {
  XYZZ *pts, *res;
  uint32_t *valid, *out;
  if (hipMalloc(&pts, SUM_TERMS * sizeof(XYZZ)) != hipSuccess || hipMalloc(&res, SUM_SLOTS * sizeof(XYZZ)) != hipSuccess ||
      hipMalloc(&valid, SUM_SLOTS * 4) != hipSuccess || hipMalloc(&out, SUM_SLOTS * 4) != hipSuccess)
    return -1;
  const uint32_t counts[] = {1, 2, 3, 5, 16, 17, 64, 128};
  int total = 0;
  for (uint32_t mix = 0; mix < 4; mix++)
    for (uint32_t n : counts) {
      static uint32_t h[SUM_SLOTS];
      if (hipMemset(valid, 0, SUM_SLOTS * 4) != hipSuccess || hipMemset(out, 0, SUM_SLOTS * 4) != hipSuccess) return -1;
      sums<<<1, 256>>>(pts, res, valid, out, n, mix);
      if (hipMemcpy(h, out, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return -1;
      const uint32_t from_d = butterfly_from(n < 16 ? n : 16);
      int want = 4 * (from_d ? from_d / 2 : 1) + 4 + 5, checks = 0, bad = 0;
      for (uint32_t width : {2u, 4u, 16u, 32u, 64u})
        for (uint32_t g = 0; g < 256 / width; g++) want += tree_group_live(width, g);
      for (uint32_t s = 0; s < SUM_SLOTS; s++) {
        checks += h[s] != 0;
        bad += h[s] == 2;
      }
      if (checks != want) bad += 1000;  // a result that was never compared
      printf("sums n %3u mix %u: %d results, %d disagree\n", n, mix, checks, bad);
      total += bad;
    }
  return total;
}

int main() {
  uint32_t* d;
  if (hipMalloc(&d, 64 * 4) != hipSuccess) return 2;
  int total = 0;
  for (uint32_t mode = 0; mode < 6; mode++) {
    test<<<1, 64>>>(d, mode);
    uint32_t h[64];
    if (hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    int bad = 0;
    for (int i = 0; i < 64; i++) bad += !h[i];
    printf("mode %u: %d of 64 lanes disagree\n", mode, bad);
    total += bad;
  }
  const int sums_bad = run_sums();
  if (sums_bad < 0) return 2;
  total += sums_bad;
  printf(total ? "FAILED\n" : "ok\n");
  return total ? 1 : 0;
}

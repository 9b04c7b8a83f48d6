// cq_pk_check_witness: `MockProver::verify` (halo2_proofs/src/dev.rs:601-958) on the GPU, over the key and the witness a
// caller is about to prove, extended to static (CQ) lookups, which the reference's MockProver ignores (dev.rs:345-350).
// Everything runs on the n rows of the Lagrange basis -- no NTT, no MSM:
//   * gates             -- the checking form of gate_eval_kernel (plonk.hip): a verdict per (polynomial, row);
//   * legacy lookups    -- input and table expressions evaluated with their poison bits, the table tuples of the usable
//                          rows put into a hash (whole tuples compared; repeated rows are expected), one probe per input row;
//   * static lookups    -- round 1's per-row verdict (cq_round1_kernel) kept per row instead of folded into one flag;
//   * permutation       -- the mapping is recovered from the key's sigma values: the PC * n identity values
//                          delta^c omega^r are hashed to their cell, every sigma value is looked up, the two cells compared.
// Verdicts are one bit per (check, row), checks ordered (kind, index): a wave's ballot writes 64 rows at once, the number
// of findings is the population count of the bitmap and the first `cap` of them come out of an ordered compaction.  With
// no findings (the common case) one counter crosses PCIe.
#include <algorithm>
#include <vector>
#include "cq.hpp"
#include "ctx.hpp"
#include "plonk.hpp"
#include "tablehash.hpp"

namespace cq {

typedef unsigned long long u64;
static inline uint32_t blocks_for(size_t n) { return (uint32_t)((n + 255) / 256); }

// ---- permutation (dev.rs:908-951) ---------------------------------------------------------------------------------
// slots[hash(delta^c omega^r)] = c * n + r.  The identity values are distinct, so an occupied slot is another value's.
__global__ __launch_bounds__(256) void perm_ident_insert_kernel(const Fr* __restrict__ delta_powers, const Fr* __restrict__ omega_powers,
                                                                uint32_t n, uint32_t* __restrict__ slots, uint32_t nslots,
                                                                uint32_t* __restrict__ err) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const uint32_t cell = blockIdx.y * n + r;
  const Fr v = ld(delta_powers + blockIdx.y) * ld(omega_powers + r);
  uint32_t s = hash_fr(v) & (nslots - 1);
  for (uint32_t probe = 0; probe < nslots; probe++) {
    if (atomicCAS(&slots[s], EMPTY, cell) == EMPTY) return;
    s = (s + 1) & (nslots - 1);
  }
  atomicExch(err, 1u);
}

// value(c, r) == value(sigma(c, r)) for every cell of the permutation columns; a sigma value that is no identity value
// (a corrupt key) is a finding on its cell
__global__ __launch_bounds__(256) void perm_check_kernel(const Fr* __restrict__ sigma, const Fr* __restrict__ delta_powers,
                                                         const Fr* __restrict__ omega_powers, const Fr* const* __restrict__ cols,
                                                         uint32_t n, uint32_t log_n, const uint32_t* __restrict__ slots, uint32_t nslots,
                                                         u64* __restrict__ fail_bits, uint32_t words) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const uint32_t c = blockIdx.y;
  const Fr sv = ld(sigma + (size_t)c * n + r);
  bool bad = false;
  if (!(sv == ld(delta_powers + c) * ld(omega_powers + r))) {  // most cells map to themselves: no probe, nothing to compare
    uint32_t found = EMPTY;
    uint32_t s = hash_fr(sv) & (nslots - 1);
    for (uint32_t probe = 0; probe < nslots; probe++) {
      const uint32_t cell = slots[s];
      if (cell == EMPTY) break;
      if (ld(delta_powers + (cell >> log_n)) * ld(omega_powers + (cell & (n - 1))) == sv) {
        found = cell;
        break;
      }
      s = (s + 1) & (nslots - 1);
    }
    bad = found == EMPTY || !(ld(cols[c] + r) == ld(cols[found >> log_n] + (found & (n - 1))));
  }
  const u64 b = __ballot(bad);
  if ((threadIdx.x & 63u) == 0) fail_bits[(size_t)c * words + (r >> 6)] = b;
}

// ---- legacy lookups (dev.rs:768-906) -------------------------------------------------------------------------------
// Expression e of the lookup (inputs 0 .. w-1, tables w .. 2w-1) on row r: vals[e * n + r], zero where its bit of
// pbits[e * words + (r >> 6)] says poisoned -- so equal tuples are equal bit for bit and hash alike.
struct TupleArgs {
  const Fr* vals;
  const u64* pbits;
  uint32_t w, n, u, words;
  uint32_t* slots;  // table row per slot
  uint32_t nslots;
};
static __device__ __forceinline__ uint32_t tuple_poison(const TupleArgs& a, uint32_t e, uint32_t row) {
  return (uint32_t)(a.pbits[(size_t)e * a.words + (row >> 6)] >> (row & 63u)) & 1u;
}
static __device__ __forceinline__ uint32_t tuple_hash(const TupleArgs& a, uint32_t e0, uint32_t row) {
  uint32_t h = 0x2545f491u;
  for (uint32_t j = 0; j < a.w; j++) {
    h = (h ^ hash_fr(ld(a.vals + (size_t)(e0 + j) * a.n + row)) ^ tuple_poison(a, e0 + j, row)) * 0x9e3779b1u;
    h ^= h >> 15;
  }
  return h;
}
static __device__ __forceinline__ bool tuple_equal(const TupleArgs& a, uint32_t e0, uint32_t row0, uint32_t e1, uint32_t row1) {
  for (uint32_t j = 0; j < a.w; j++) {
    if (tuple_poison(a, e0 + j, row0) != tuple_poison(a, e1 + j, row1)) return false;
    if (!(ld(a.vals + (size_t)(e0 + j) * a.n + row0) == ld(a.vals + (size_t)(e1 + j) * a.n + row1))) return false;
  }
  return true;
}
// the table tuples of the usable rows; a tuple that is already there (padding rows repeat) is left alone
__global__ __launch_bounds__(256) void tuple_insert_kernel(TupleArgs a, uint32_t* __restrict__ err) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.u) return;
  uint32_t s = tuple_hash(a, a.w, r) & (a.nslots - 1);
  for (uint32_t probe = 0; probe < a.nslots; probe++) {
    const uint32_t prev = atomicCAS(&a.slots[s], EMPTY, r);
    if (prev == EMPTY || tuple_equal(a, a.w, r, a.w, prev)) return;
    s = (s + 1) & (a.nslots - 1);
  }
  atomicExch(err, 1u);
}
__global__ __launch_bounds__(256) void tuple_probe_kernel(TupleArgs a, u64* __restrict__ fail_bits) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n) return;
  bool bad = false;
  if (r < a.u) {
    bad = true;
    uint32_t s = tuple_hash(a, 0, r) & (a.nslots - 1);
    for (uint32_t probe = 0; probe < a.nslots; probe++) {
      const uint32_t row = a.slots[s];
      if (row == EMPTY) break;
      if (tuple_equal(a, 0, r, a.w, row)) {
        bad = false;
        break;
      }
      s = (s + 1) & (a.nslots - 1);
    }
  }
  const u64 b = __ballot(bad);
  if ((threadIdx.x & 63u) == 0) fail_bits[r >> 6] = b;
}

// ---- static lookups (static_lookup/prover.rs:132-161, per row) -------------------------------------------------------
struct StaticCheckArgs {
  const Fr* cols[CQ_MAX_WIDTH];     // input values, n each: an advice column or an evaluated expression
  const u64* pbits[CQ_MAX_WIDTH];   // poison bits of an evaluated expression; nullptr for an advice column (usable rows are real)
  const Fr* values[CQ_MAX_WIDTH];
  const uint32_t* slots[CQ_MAX_WIDTH];
  uint32_t nslots[CQ_MAX_WIDTH];
  uint32_t width;
};
__global__ __launch_bounds__(256) void static_check_kernel(StaticCheckArgs a, uint32_t n, uint32_t u, u64* __restrict__ fail_bits,
                                                           uint8_t* __restrict__ detail) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  bool bad = false;
  uint32_t why = 0, idx = EMPTY;
  for (uint32_t j = 0; r < u && !bad && j < a.width; j++) {
    if (a.pbits[j] && ((a.pbits[j][r >> 6] >> (r & 63u)) & 1ull)) {
      bad = true;
      why = 2;  // the prover would look up a blinding value it draws at random
      break;
    }
    const uint32_t ix = table_find(a.values[j], a.slots[j], a.nslots[j], ld(a.cols[j] + r));
    if (ix == EMPTY) {
      bad = true;
      why = 0;  // "{:?} not in table" (:141)
    } else if (j && ix != idx) {
      bad = true;
      why = 1;  // "Vector lookup must be on the same table row" (:148)
    }
    idx = ix;
  }
  if (bad) detail[r] = (uint8_t)why;
  const u64 b = __ballot(bad);
  if ((threadIdx.x & 63u) == 0) fail_bits[r >> 6] = b;
}

// ---- counting and ordered compaction of the verdict bitmap -------------------------------------------------------------
// inclusive sum scan of one value per lane across the 256-lane block (Hillis-Steele in LDS)
static __device__ __forceinline__ uint32_t block_scan_sum(uint32_t v, uint32_t* sh) {
  const uint32_t t = threadIdx.x;
#pragma unroll 1
  for (uint32_t d = 1; d < 256; d <<= 1) {
    sh[t] = v;
    __syncthreads();
    if (t >= d) v += sh[t - d];
    __syncthreads();
  }
  return v;
}
__global__ __launch_bounds__(256) void bits_count_kernel(const u64* __restrict__ bits, uint32_t nwords, uint32_t* __restrict__ block_sums,
                                                         u64* __restrict__ total) {
  __shared__ uint32_t sh[256];
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  const uint32_t inc = block_scan_sum(g < nwords ? (uint32_t)__popcll(bits[g]) : 0u, sh);
  if (threadIdx.x == 255) {
    block_sums[blockIdx.x] = inc;
    if (inc) atomicAdd(total, (u64)inc);
  }
}
// exclusive scan of the block sums, 256 at a time with a running carry (one block)
__global__ __launch_bounds__(256) void bits_spine_kernel(uint32_t* __restrict__ block_sums, uint32_t nblocks) {
  __shared__ uint32_t sh[256];
  const uint32_t t = threadIdx.x;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nblocks; base += 256) {
    const uint32_t v = base + t < nblocks ? block_sums[base + t] : 0u;
    const uint32_t inc = block_scan_sum(v, sh);
    sh[t] = inc;
    __syncthreads();
    const uint32_t tile = sh[255];
    __syncthreads();
    if (base + t < nblocks) block_sums[base + t] = carry + inc - v;
    carry += tile;
  }
}
struct CheckLayout {
  uint32_t gates, legacy, statics, perms;  // checks in bitmap order: gates failed | gates poisoned | legacy | static | permutation
  uint32_t words, n;
  const uint8_t* detail;                   // statics x n
};
__global__ __launch_bounds__(256) void bits_emit_kernel(const u64* __restrict__ bits, uint32_t nwords, const uint32_t* __restrict__ block_offsets,
                                                        CheckLayout lay, uint32_t cap, uint4* __restrict__ out) {
  __shared__ uint32_t sh[256];
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  u64 w = g < nwords ? bits[g] : 0ull;
  const uint32_t cnt = (uint32_t)__popcll(w);
  uint32_t pos = block_offsets[blockIdx.x] + block_scan_sum(cnt, sh) - cnt;
  if (!w || pos >= cap) return;
  uint32_t check = g / lay.words, kind, index = check;
  const uint32_t row0 = (g % lay.words) * 64;
  if (index < lay.gates) {
    kind = CQ_FAIL_GATE;
  } else if ((index -= lay.gates) < lay.gates) {
    kind = CQ_FAIL_GATE_POISONED;
  } else if ((index -= lay.gates) < lay.legacy) {
    kind = CQ_FAIL_LOOKUP;
  } else if ((index -= lay.legacy) < lay.statics) {
    kind = CQ_FAIL_STATIC_LOOKUP;
  } else {
    index -= lay.statics;
    kind = CQ_FAIL_PERMUTATION;
  }
  for (; w && pos < cap; w &= w - 1, pos++) {
    const uint32_t row = row0 + (uint32_t)__ffsll((long long)w) - 1;
    out[pos] = make_uint4(kind, index, row, kind == CQ_FAIL_STATIC_LOOKUP ? lay.detail[(size_t)index * lay.n + row] : 0u);
  }
}

}  // namespace cq

using namespace cq;

#define CHECK_TRY(x)                   \
  do {                                 \
    const int _rc = (x);               \
    if (_rc != CQ_OK) return _rc;      \
  } while (0)
#define CHECK_LAUNCHED(what) \
  if (hipGetLastError() != hipSuccess) return c->fail(CQ_ERR_HIP, what " launch failed")

namespace {
// carves the one Scratch::Check allocation: sizes are collected first, pointers handed out after it exists
struct Carver {
  size_t total = 0;
  size_t take(size_t bytes) {
    const size_t off = total;
    total += (bytes + 255) & ~(size_t)255;
    return off;
  }
};
uint32_t pow2_at_least(size_t x) {
  uint32_t p = 64;
  while (p < x) p <<= 1;
  return p;
}
}  // namespace

extern "C" int cq_pk_check_witness(cq_pk* pk, const uint64_t* const* advice, int advice_on_device, const uint64_t* const* instances,
                                   const size_t* instance_lens, const uint64_t* challenges, cq_witness_failure* failures, size_t cap,
                                   size_t* total_out) {
  if (!pk || !total_out || (!advice && pk->num_advice) || (cap && !failures)) return CQ_ERR_ARG;
  cq_ctx* c = pk->ctx;
  const size_t A = pk->num_advice, I = pk->num_instance, NC = pk->challenge_phase.size();
  const size_t G = pk->num_gate_polys, PL = pk->legacy.size(), L = pk->lookups.size(), PC = pk->perm_columns.size();
  const size_t n = (size_t)1 << pk->k, u = pk->u;
  if (pk->shard_world > 1) return c->fail(CQ_ERR_ARG, "check_witness: the key is sharded");
  if (I && (!instances || !instance_lens)) return c->fail(CQ_ERR_ARG, "check_witness: instance columns missing");
  for (size_t i = 0; i < I; i++)
    if (instance_lens[i] > u) return c->fail(CQ_ERR_ARG, "Error::InstanceTooLarge");  // prover.rs:108-110
  if (NC && !challenges) return c->fail(CQ_ERR_ARG, "check_witness: the circuit has challenges and none were given");
  for (size_t a = 0; a < A; a++)
    if (!advice[a]) return c->fail(CQ_ERR_ARG, "check_witness: null advice column");
  CQ_HIP(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  *total_out = 0;

  const size_t checks = 2 * G + PL + L + PC;
  if (!checks) return CQ_OK;
  const size_t words = (n + 63) / 64, nwords = checks * words;
  if (checks * n >= ((size_t)1 << 32)) return c->fail(CQ_ERR_ARG, "check_witness: too many (constraint, row) pairs");
  const size_t nblocks = (nwords + 255) / 256;
  // expression values kept at a time: one legacy lookup's inputs and tables, or one static lookup's expression inputs
  size_t max_exprs = 0;
  for (auto& lk : pk->legacy) max_exprs = std::max<size_t>(max_exprs, 2 * (size_t)lk.width);
  for (auto& lk : pk->lookups) {
    size_t e = 0;
    for (int64_t p : lk.prog) e += p >= 0;
    max_exprs = std::max(max_exprs, e);
  }
  const uint32_t perm_slots = PC ? pow2_at_least(2 * PC * n) : 0, tuple_slots = PL ? pow2_at_least(2 * u) : 0;
  const size_t out_cap = std::min<size_t>(cap, checks * n);

  Carver cv;
  const size_t o_adv = cv.take(A * n * sizeof(Fr)), o_inst = cv.take(I * n * sizeof(Fr)), o_chal = cv.take((NC + 1) * sizeof(Fr));
  const size_t o_bits = cv.take(nwords * sizeof(u64)), o_detail = cv.take(L * n);
  const size_t o_vals = cv.take(max_exprs * n * sizeof(Fr)), o_pbits = cv.take(max_exprs * words * sizeof(u64));
  const size_t o_slots = cv.take((size_t)std::max(perm_slots, tuple_slots) * sizeof(uint32_t));
  const size_t o_cols = cv.take(PC * sizeof(Fr*)), o_dp = cv.take(PC * sizeof(Fr));
  const size_t o_sums = cv.take(nblocks * sizeof(uint32_t)), o_total = cv.take(16), o_out = cv.take(out_cap * sizeof(uint4));
  void* base_v;
  CHECK_TRY(c->ensure_scratch(Scratch::Check, cv.total, &base_v));
  char* base = (char*)base_v;
  Fr *adv = (Fr*)(base + o_adv), *inst = (Fr*)(base + o_inst), *chal = (Fr*)(base + o_chal), *vals = (Fr*)(base + o_vals);
  u64 *bits = (u64*)(base + o_bits), *pbits = (u64*)(base + o_pbits), *total_dev = (u64*)(base + o_total);
  uint32_t *slots = (uint32_t*)(base + o_slots), *sums = (uint32_t*)(base + o_sums), *err_dev = (uint32_t*)(base + o_total + 8);
  uint8_t* detail = (uint8_t*)(base + o_detail);

  // ---- the witness as the prover reads it: rows [0, usable) of every advice column; what the caller left in the
  //      blinding rows is dropped here (zeros), so host and device advice are checked alike --------------------------
  for (size_t a = 0; a < A; a++) {
    CQ_HIP(c, hipMemcpyAsync(adv + a * n, advice[a], u * sizeof(Fr), advice_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    CQ_HIP(c, hipMemsetAsync(adv + a * n + u, 0, (n - u) * sizeof(Fr), s));
  }
  if (I) CQ_HIP(c, hipMemsetAsync(inst, 0, I * n * sizeof(Fr), s));
  for (size_t i = 0; i < I; i++)
    if (instance_lens[i]) CQ_HIP(c, hipMemcpyAsync(inst + i * n, instances[i], instance_lens[i] * sizeof(Fr), hipMemcpyHostToDevice, s));
  if (NC) CQ_HIP(c, hipMemcpyAsync(chal, challenges, NC * sizeof(Fr), hipMemcpyHostToDevice, s));
  CQ_HIP(c, hipMemsetAsync(bits, 0, nwords * sizeof(u64), s));
  CQ_HIP(c, hipMemsetAsync(total_dev, 0, 16, s));
  if (L) CQ_HIP(c, hipMemsetAsync(detail, 0, L * n, s));

  // delta^c and the value column behind every permutation column (host vectors: alive until the call's last synchronise)
  std::vector<Fr> dp(PC);
  std::vector<const Fr*> cols(PC);
  Fr* dp_dev = (Fr*)(base + o_dp);
  const Fr** cols_dev = (const Fr**)(base + o_cols);
  if (PC) {
    const Fr delta = fr_from_raw(FR_DELTA_RAW);
    Fr cur = Fr::one();
    for (size_t q = 0; q < PC; q++) {
      dp[q] = cur;
      cur = cur * delta;
      const uint32_t kind = pk->perm_columns[q].first, idx = pk->perm_columns[q].second;
      cols[q] = (kind == CQ_COL_ADVICE ? adv : kind == CQ_COL_FIXED ? pk->fixed_values : inst) + (size_t)idx * n;
    }
    CQ_HIP(c, hipMemcpyAsync(dp_dev, dp.data(), PC * sizeof(Fr), hipMemcpyHostToDevice, s));
    CQ_HIP(c, hipMemcpyAsync(cols_dev, cols.data(), PC * sizeof(Fr*), hipMemcpyHostToDevice, s));
  }

  GateCheckArgs ga;
  ga.constants = pk->constants;
  ga.challenges = chal;
  ga.advice = adv;
  ga.fixed = pk->fixed_values;
  ga.instance = inst;
  ga.stride = n;
  ga.size = (uint32_t)n;
  ga.rot_scale = 1;
  ga.y = Fr::zero();
  ga.usable = (uint32_t)u;
  ga.words = (uint32_t)words;

  // ---- gates (dev.rs:694-766): bitmap checks [0, G) failed, [G, 2G) poisoned ----------------------------------------
  if (G) {
    ga.prog = pk->gate_prog;
    ga.num_polys = (uint32_t)G;
    ga.fail_bits = bits;
    ga.poison_bits = bits + G * words;
    CHECK_TRY(gate_check(c, ga, nullptr));
  }
  ga.fail_bits = nullptr;
  ga.poison_bits = pbits;

  // ---- legacy lookups (dev.rs:768-906) ---------------------------------------------------------------------------------
  for (size_t l = 0; l < PL; l++) {
    const cq_pk::LegacyLookup& lk = pk->legacy[l];
    ga.prog = pk->legacy_prog + lk.in_off;  // the w input programs, then the w table programs
    ga.num_polys = 2 * lk.width;
    CHECK_TRY(gate_check(c, ga, vals));
    TupleArgs ta;
    ta.vals = vals;
    ta.pbits = pbits;
    ta.w = lk.width;
    ta.n = (uint32_t)n;
    ta.u = (uint32_t)u;
    ta.words = (uint32_t)words;
    ta.slots = slots;
    ta.nslots = tuple_slots;
    CQ_HIP(c, hipMemsetAsync(slots, 0xff, (size_t)tuple_slots * sizeof(uint32_t), s));
    tuple_insert_kernel<<<blocks_for(u), 256, 0, s>>>(ta, err_dev);
    tuple_probe_kernel<<<blocks_for(n), 256, 0, s>>>(ta, bits + (2 * G + l) * words);
    CHECK_LAUNCHED("check_witness: legacy lookup");
  }

  // ---- static lookups (static_lookup/prover.rs:91-107, 132-161) ------------------------------------------------------------
  for (size_t l = 0; l < L; l++) {
    const cq_lookup_desc& lk = pk->lookups[l];
    StaticCheckArgs sa;
    sa.width = (uint32_t)lk.cols.size();
    size_t e = 0;
    for (uint32_t j = 0; j < sa.width; j++) {
      sa.values[j] = lk.tables[j]->values;
      sa.slots[j] = lk.tables[j]->slots;
      sa.nslots[j] = lk.tables[j]->nslots;
      if (lk.prog[j] < 0) {  // advice[col] @ Rotation::cur(): read in place, as round 1 does
        sa.cols[j] = adv + (size_t)lk.cols[j] * n;
        sa.pbits[j] = nullptr;
        continue;
      }
      ga.prog = pk->lookup_prog + lk.prog[j];
      ga.num_polys = 1;
      ga.poison_bits = pbits + e * words;
      CHECK_TRY(gate_check(c, ga, vals + e * n));
      sa.cols[j] = vals + e * n;
      sa.pbits[j] = pbits + e * words;
      e++;
    }
    static_check_kernel<<<blocks_for(n), 256, 0, s>>>(sa, (uint32_t)n, (uint32_t)u, bits + (2 * G + PL + l) * words, detail + l * n);
    CHECK_LAUNCHED("check_witness: static lookup");
  }

  // ---- permutation (dev.rs:908-951) -----------------------------------------------------------------------------------------
  if (PC) {
    CQ_HIP(c, hipMemsetAsync(slots, 0xff, (size_t)perm_slots * sizeof(uint32_t), s));
    uint32_t log_n = pk->k;
    perm_ident_insert_kernel<<<dim3(blocks_for(n), (uint32_t)PC), 256, 0, s>>>(dp_dev, pk->omega_powers, (uint32_t)n, slots, perm_slots, err_dev);
    perm_check_kernel<<<dim3(blocks_for(n), (uint32_t)PC), 256, 0, s>>>(pk->perm_values, dp_dev, pk->omega_powers, cols_dev, (uint32_t)n, log_n,
                                                                       slots, perm_slots, bits + (2 * G + PL + L) * words, (uint32_t)words);
    CHECK_LAUNCHED("check_witness: permutation");
  }

  // ---- count; then the first `cap` findings in bitmap order = (kind, index, row) ascending ----------------------------------
  bits_count_kernel<<<(uint32_t)nblocks, 256, 0, s>>>(bits, (uint32_t)nwords, sums, total_dev);
  CHECK_LAUNCHED("check_witness: count");
  u64 counters[2] = {0, 0};  // total, hash-full flag
  CQ_HIP(c, hipMemcpyAsync(counters, total_dev, 16, hipMemcpyDeviceToHost, s));
  CQ_HIP(c, hipStreamSynchronize(s));
  if ((uint32_t)counters[1]) return c->fail(CQ_ERR_INTERNAL, "check_witness: hash table full");
  *total_out = (size_t)counters[0];
  const size_t take = std::min<size_t>(cap, (size_t)counters[0]);
  if (!take) return CQ_OK;
  CheckLayout lay;
  lay.gates = (uint32_t)G;
  lay.legacy = (uint32_t)PL;
  lay.statics = (uint32_t)L;
  lay.perms = (uint32_t)PC;
  lay.words = (uint32_t)words;
  lay.n = (uint32_t)n;
  lay.detail = detail;
  uint4* out_dev = (uint4*)(base + o_out);
  bits_spine_kernel<<<1, 256, 0, s>>>(sums, (uint32_t)nblocks);
  bits_emit_kernel<<<(uint32_t)nblocks, 256, 0, s>>>(bits, (uint32_t)nwords, sums, lay, (uint32_t)take, out_dev);
  CHECK_LAUNCHED("check_witness: compaction");
  CQ_HIP(c, hipMemcpyAsync(failures, out_dev, take * sizeof(cq_witness_failure), hipMemcpyDeviceToHost, s));
  CQ_HIP(c, hipStreamSynchronize(s));
  return CQ_OK;
}

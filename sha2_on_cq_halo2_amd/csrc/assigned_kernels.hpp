// The kernels of batch_invert_assigned over Assigned columns (poly.hpp: poly_resolve_assigned, poly_validate_assigned).
// Part of poly.hip's translation unit -- included there behind batch_invert_block and the load / store helpers it uses --
// and of no other: the text below sits inside poly.hip's `namespace cq`.
#pragma once

// ---- batch_invert_assigned(_ref) (poly.rs:174-241): the rational cells of Assigned columns -----------------------------
// A column arrives as its numerators (dense: Zero -> 0, Trivial(x) -> x, Rational(a, b) -> a; assigned.rs:281-287) and the
// rows and denominators of its Rational cells only (:290-296, "if the denominator is trivial, we can skip it",
// poly.rs:189-191), the columns' lists back to back: entry i belongs to the column c with off[c] <= i < off[c + 1] and names
// the cell out[c][rows[i]] = num[c][rows[i]] / den[i], or 0 where den[i] is zero (assigned.rs:353-366; BatchInvert leaves
// zeros at zero).  An entry whose row is not below `nrows` names no cell and is never dereferenced.  The kernels that
// write do nothing once `verdict` (may be null) holds an entry: a list that failed its check leaves the output as it was.
static __device__ __forceinline__ uint32_t assigned_column_of(const AssignedCols& cols, uint32_t i) {
  uint32_t c = 0;  // the last column that starts at or before i: empty columns before it start there too
  CQ_UNROLL for (uint32_t step = ASSIGNED_MAX_COLS / 2; step; step >>= 1)
    if (c + step < cols.count && cols.off[c + step] <= i) c += step;
  return c;
}
static __device__ __forceinline__ bool assigned_gate_shut(const uint32_t* verdict) { return verdict && *verdict != 0xffffffffu; }

// entry i is bad when its row is not below nrows or not above the row of the entry before it in the same column
__global__ __launch_bounds__(256) void assigned_validate_kernel(AssignedCols cols, const uint32_t* __restrict__ rows, uint32_t nrows,
                                                                uint32_t entry_base, uint32_t* verdict) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cols.off[cols.count]) return;
  const uint32_t c = assigned_column_of(cols, i), row = rows[i];
  if (row >= nrows || (i > cols.off[c] && rows[i - 1] >= row)) atomicMin(verdict, entry_base + i);
}
// one 16-byte half element per lane: the cells no entry names, for a column whose output is not its numerator array
__global__ __launch_bounds__(256) void assigned_copy_kernel(AssignedCols cols, uint32_t nrows, const uint32_t* verdict) {
  const uint32_t col = blockIdx.y;
  const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= 2 * nrows || cols.out[col] == cols.num[col] || assigned_gate_shut(verdict)) return;
  reinterpret_cast<uint4*>(cols.out[col])[h] = reinterpret_cast<const uint4*>(cols.num[col])[h];
}
// batch_invert_block's IO for the fused form: elements from the denominator list, prefix products parked in `work`, results
// times numerator straight into the cells
struct BiResolve {
  static constexpr bool kNumerator = true;
  const AssignedCols& cols;
  const uint32_t* __restrict__ rows;
  const Fr* __restrict__ den;
  Fr* __restrict__ work;
  uint32_t nrows;
  struct Cell {
    const Fr* num;  // null: the entry names no cell
    Fr* out;
    __device__ __forceinline__ Fr29 numerator() const {
      uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (num) ld8w(num, w);
      return Fr29::unpack(w);
    }
    __device__ __forceinline__ void emit(bool nz, const Fr29& x) const {  // x = numerator / denominator (< 2 p); x / 0 = 0
      if (!num) return;
      uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (nz) {
        x.pack(w);
        Fr::cond_sub_p(w, 0);
      }
      uint4* dst = reinterpret_cast<uint4*>(out);
      dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
      dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
    }
  };
  // inverse (x) numerator, two memory words, is the quotient's word over 32 on the R' = 2^261 limbs: the lane's "before"
  // products carry the 32 (as 2^266 / R').  Bound: x < 2 p times a constant < p.
  static __device__ __forceinline__ Fr29 scaled_for_numerator(const Fr29& x) {
    Fr29 c32;
    CQ_UNROLL for (int q = 0; q < 9; q++) c32.a[q] = CONSTS29<FrP>.from256[q];
    return Fr29::mul(x, c32);
  }
  // o <- o (x) numerator for two cells at once.  Bound: o < 2 p times any memory word (< 2^256 < 6 p, limbs < 2^29).
  static __device__ __forceinline__ void times_numerators(const Cell& c1, Fr29& o1, const Cell& c0, Fr29& o0) {
    Fr29::mul_pair(o1, c1.numerator(), o0, c0.numerator(), o1, o0);
  }
  __device__ __forceinline__ void load(uint32_t i, uint32_t* w) const { ld8w(den + i, w); }
  __device__ __forceinline__ Fr* slot(uint32_t i) const { return work + i; }
  __device__ __forceinline__ Cell cell(uint32_t i, uint32_t n) const {
    Cell r{nullptr, nullptr};
    if (i < n) {
      const uint32_t c = assigned_column_of(cols, i), row = rows[i];
      if (row < nrows) r = Cell{cols.num[c] + row, cols.out[c] + row};
    }
    return r;
  }
};
template <int BI_PER_LANE>
__global__ __launch_bounds__(256) void assigned_resolve_kernel(AssignedCols cols, const uint32_t* __restrict__ rows, const Fr* __restrict__ den,
                                                               Fr* __restrict__ work, uint32_t nrows, const uint32_t* verdict) {
  CQ_CRITICAL_WAVES();
  if (assigned_gate_shut(verdict)) return;
  batch_invert_block<BI_PER_LANE>(BiResolve{cols, rows, den, work, nrows}, cols.off[cols.count]);
}

// Host side of proving-key construction (pk.hip): the description of a key -- every field that is lowered from the caller's
// cq_circuit / cq_plonk without the GPU -- the function that validates and fills it, and the packing of expression programs.
// No HIP here: tests/host/pk_describe_check.cpp builds this header alone, under the host sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>
#include "../../include/cq_halo2.h"

namespace cq {
// The two things pk_describe asks of the rest of the library (pk.hip, plonk.hip); the host check links stand-ins.
size_t static_table_rows(const cq_static_table* t);
bool gate_program_check(const uint32_t* lens, const uint32_t* words, uint32_t num_polys, uint32_t num_constants,
                        uint32_t num_advice, uint32_t num_fixed, uint32_t num_instance, uint32_t num_challenges,
                        const char** why, size_t* total_words);
}  // namespace cq

struct cq_lookup_desc {
  std::vector<uint32_t> cols;             // advice column per table column (input = advice[col] @ Rotation::cur())
  std::vector<int64_t> prog;              // or: word offset of the input's program in cq_pk::lookup_prog (-1 = plain column)
  std::vector<cq_static_table*> tables;
};

// The host fields of cq_pk (cq.hpp), all of them filled by pk_describe
struct cq_pk_desc {
  uint32_t k = 0, num_advice = 0, bf = 0, u = 0;
  std::vector<cq_lookup_desc> lookups;
  std::vector<std::pair<uint32_t, int32_t>> advice_queries;  // (column, rotation), registration order
  // ---- general PLONK part (empty for a CQ-only circuit) ----
  uint32_t num_fixed = 0, num_instance = 0, cs_degree = 3;
  std::vector<std::pair<uint32_t, int32_t>> fixed_queries;
  uint32_t num_gate_polys = 0;
  bool lookup_exprs = false;  // the lookup inputs are expressions: lookups[l].prog[j] names their programs
  // legacy lookups: per lookup the number of (input, table) expression pairs and the word offsets of the two
  // program lists ([len, words...] x width each) in `legacy_prog`
  struct LegacyLookup { uint32_t width; size_t in_off, tab_off; };
  std::vector<LegacyLookup> legacy;
  std::vector<std::pair<uint32_t, uint32_t>> perm_columns;  // (CQ_COL_*, index) = cs.permutation.columns
  std::vector<uint8_t> advice_phase;     // phase of every advice column
  std::vector<uint8_t> challenge_phase;  // phase after which user challenge i is squeezed
  uint32_t num_phases = 1;
  bool general() const { return num_gate_polys || !perm_columns.empty() || !legacy.empty(); }
  size_t perm_sets() const {
    const size_t chunk = cs_degree - 2;
    return (perm_columns.size() + chunk - 1) / chunk;
  }
  // The multi-open groups queries by their POINT (gwc.rs:36-61, shplonk.rs:56-133), and omega^rot x is the same point for
  // every rotation of one residue modulo 2^k: the representative in [-n/2, n/2) stands for all of them.
  int32_t point_rotation(int32_t rot) const {
    const int64_t n = (int64_t)1 << k, r = (((int64_t)rot % n) + n) % n;
    return (int32_t)(r >= (n + 1) / 2 ? r - n : r);
  }
  // the distinct points the proof opens at, as rotations of x: one GWC witness each, one evaluation batch each
  std::vector<int32_t> opening_rotations() const {
    std::vector<int32_t> rots{0};
    auto seen = [&](int32_t rot) {
      const int32_t r = point_rotation(rot);
      if (std::find(rots.begin(), rots.end(), r) == rots.end()) rots.push_back(r);
    };
    for (auto& q : advice_queries) seen(q.second);
    for (auto& q : fixed_queries) seen(q.second);
    if (perm_sets() || !legacy.empty()) seen(1);
    if (!legacy.empty()) seen(-1);
    if (perm_sets() > 1) seen(-(int32_t)(bf + 1));
    return rots;
  }
};

namespace cq {

// capacities of the kernels' argument structs (poly.hpp, cq.hpp, plonk.hpp), handed in so that this header stays free of them
struct PkLimits {
  uint32_t lookups, width, perm_columns, perm_chunk;
};

// Program i of a list becomes [lens[i], its words...] in one blob, the form the interpreters read; offsets[i] = the word at
// which it starts.
inline std::vector<uint32_t> pack_programs(const uint32_t* lens, const uint32_t* words, size_t count, std::vector<size_t>* offsets = nullptr) {
  std::vector<uint32_t> blob;
  for (size_t i = 0; i < count; i++) {
    if (offsets) offsets->push_back(blob.size());
    blob.push_back(lens[i]);
    blob.insert(blob.end(), words, words + lens[i]);
    words += lens[i];
  }
  return blob;
}

// The three program blobs of a described key, as they go to the device; writes the word offsets into `d`: legacy lookup l's
// input list at in_off and table list at tab_off, lookup input (l, j) at lookups[l].prog[j].
struct PkPrograms {
  std::vector<uint32_t> gates, legacy, lookups;
};
inline PkPrograms pk_pack_programs(const cq_plonk* pl, cq_pk_desc* d) {
  PkPrograms out;
  if (d->num_gate_polys) out.gates = pack_programs(pl->gate_program_lens, pl->gate_programs, d->num_gate_polys);
  std::vector<size_t> at;
  size_t count = 0, i = 0;
  for (auto& lk : d->legacy) count += 2 * (size_t)lk.width;
  if (count) out.legacy = pack_programs(pl->legacy_program_lens, pl->legacy_programs, count, &at);
  for (auto& lk : d->legacy) {
    lk.in_off = at[i];
    lk.tab_off = at[i + lk.width];
    i += 2 * (size_t)lk.width;
  }
  if (d->lookup_exprs) {
    at.clear();
    count = i = 0;
    for (auto& lk : d->lookups) count += lk.cols.size();
    out.lookups = pack_programs(pl->lookup_input_program_lens, pl->lookup_input_programs, count, &at);
    for (auto& lk : d->lookups)
      for (auto& at_word : lk.prog) at_word = (int64_t)at[i++];
  }
  return out;
}

inline int pk_reject(std::string* err, const char* why) {
  *err = why;
  return CQ_ERR_ARG;
}

// pk_describe's part for a general circuit: queries, phases, permutation columns, then the three lists of expression programs
inline int pk_describe_plonk(const cq_circuit* cs, size_t lookup_inputs, bool from_stream, const PkLimits& lim, cq_pk_desc* d, std::string* err) {
  auto fail = [&](const char* why) { return pk_reject(err, why); };
  const cq_plonk* pl = cs->plonk;
  d->num_fixed = pl->num_fixed;
  d->num_instance = pl->num_instance;
  d->cs_degree = pl->cs_degree ? pl->cs_degree : 3;
  if (d->cs_degree < 3 || d->cs_degree - 2 > lim.perm_chunk) return fail("pk: cs_degree out of range");
  if (pl->num_perm_columns > lim.perm_columns) return fail("pk: too many permutation columns");
  if ((pl->num_fixed && !pl->fixed && !from_stream) || (pl->num_gate_polys && (!pl->gate_program_lens || !pl->gate_programs)) ||
      (pl->num_constants && !pl->constants) || (pl->num_perm_columns && (!pl->perm_column_kinds || !pl->perm_column_indices)))
    return fail("pk: null pointer in cq_plonk");
  for (uint32_t q = 0; q < pl->num_advice_queries; q++) {
    if (pl->advice_query_columns[q] >= cs->num_advice) return fail("pk: advice query column out of range");
    d->advice_queries.push_back({pl->advice_query_columns[q], pl->advice_query_rotations[q]});
  }
  for (uint32_t q = 0; q < pl->num_fixed_queries; q++) {
    if (pl->fixed_query_columns[q] >= pl->num_fixed) return fail("pk: fixed query column out of range");
    d->fixed_queries.push_back({pl->fixed_query_columns[q], pl->fixed_query_rotations[q]});
  }
  // phases (circuit.rs advice_column_phase / challenge_phase)
  d->advice_phase.assign(cs->num_advice, 0);
  for (uint32_t a = 0; a < cs->num_advice && pl->advice_column_phases; a++) d->advice_phase[a] = pl->advice_column_phases[a];
  if (pl->num_challenges && !pl->challenge_phases) return fail("pk: null pointer in cq_plonk");
  d->challenge_phase.assign(pl->challenge_phases, pl->challenge_phases + pl->num_challenges);
  for (uint8_t ph : d->advice_phase) d->num_phases = std::max<uint32_t>(d->num_phases, ph + 1u);
  for (uint8_t ph : d->challenge_phase) d->num_phases = std::max<uint32_t>(d->num_phases, ph + 1u);
  if (d->num_phases > 3) return fail("pk: the API only supports 3 phases (prover.rs:337)");
  for (uint32_t q = 0; q < pl->num_perm_columns; q++) {
    const uint32_t kind = pl->perm_column_kinds[q], idx = pl->perm_column_indices[q];
    const uint32_t bound = kind == CQ_COL_ADVICE ? cs->num_advice : kind == CQ_COL_FIXED ? pl->num_fixed : kind == CQ_COL_INSTANCE ? pl->num_instance : 0;
    if (idx >= bound) return fail("pk: permutation column out of range");
    d->perm_columns.push_back({kind, idx});
  }
  // ---- expression programs: gates, legacy lookups, static lookup inputs ----
  const char* why = nullptr;
  size_t words = 0;
  auto programs_ok = [&](const uint32_t* lens, const uint32_t* prog, size_t count) {
    return gate_program_check(lens, prog, (uint32_t)count, pl->num_constants, cs->num_advice, pl->num_fixed, pl->num_instance,
                              pl->num_challenges, &why, &words);
  };
  if (pl->num_gate_polys && !programs_ok(pl->gate_program_lens, pl->gate_programs, pl->num_gate_polys)) return fail(why);
  d->num_gate_polys = pl->num_gate_polys;
  if (pl->num_legacy_lookups) {
    if (!pl->legacy_lookup_widths || !pl->legacy_program_lens || !pl->legacy_programs) return fail("pk: null pointer in cq_plonk");
    size_t nprog = 0;
    for (uint32_t l = 0; l < pl->num_legacy_lookups; l++) {
      if (pl->legacy_lookup_widths[l] == 0 || pl->legacy_lookup_widths[l] > 64) return fail("pk: legacy lookup width out of range");
      nprog += 2 * (size_t)pl->legacy_lookup_widths[l];
    }
    if (!programs_ok(pl->legacy_program_lens, pl->legacy_programs, nprog)) return fail(why);
    for (uint32_t l = 0; l < pl->num_legacy_lookups; l++) d->legacy.push_back({pl->legacy_lookup_widths[l], 0, 0});
  }
  if (pl->lookup_input_program_lens && lookup_inputs) {  // static lookup inputs given as expressions: one single-polynomial program each
    if (!pl->lookup_input_programs) return fail("pk: null pointer in cq_plonk");
    if (!programs_ok(pl->lookup_input_program_lens, pl->lookup_input_programs, lookup_inputs)) return fail(why);
    d->lookup_exprs = true;
  }
  return CQ_OK;
}

// Lowers the circuit description into `d`, or says in `err` why it cannot be a key (CQ_ERR_ARG).  Every argument check of key
// construction is here, in one order: the first that applies is the one reported.  table_rows: rows of the table config
// (nullptr: none); from_stream: the polynomials come from a serialized key, so plonk->fixed / perm_mapping are not read.
inline int pk_describe(const cq_circuit* cs, uint32_t params_k, const size_t* table_rows, bool have_b0, bool from_stream, const PkLimits& lim,
                       cq_pk_desc* d, std::string* err) {
  auto fail = [&](const char* why) { return pk_reject(err, why); };
  if (cs->num_lookups && (!table_rows || !have_b0)) return fail("pk: static lookups need a table config and b0_g1_bound");
  if (cs->k != params_k) return fail("pk: circuit k differs from params k");
  if (cs->num_lookups > lim.lookups) return fail("pk: too many lookups");
  const cq_plonk* pl = cs->plonk;
  d->k = cs->k;
  d->num_advice = cs->num_advice;
  const size_t n = (size_t)1 << d->k;
  const bool is_expr = pl && pl->lookup_input_program_lens;
  size_t off = 0;
  for (uint32_t l = 0; l < cs->num_lookups; l++) {
    cq_lookup_desc lk;
    const uint32_t w = cs->lookup_widths[l];
    if (w == 0 || w > lim.width) return fail("pk: lookup width out of range");
    for (uint32_t j = 0; j < w; j++) {
      const uint32_t col = cs->lookup_columns[off + j];
      cq_static_table* t = cs->lookup_tables[off + j];
      if ((!is_expr && col >= cs->num_advice) || !t) return fail("pk: bad lookup column / table");
      // "Tables should all be of the same size" (static_lookup/prover.rs:81-83)
      if (static_table_rows(t) != *table_rows) return fail("pk: table size differs from the table config");
      lk.cols.push_back(col);
      lk.prog.push_back(-1);
      lk.tables.push_back(t);
      // query_advice_index (plonk/circuit.rs:1619-1633)
      if (!(pl && pl->num_advice_queries) && !is_expr &&
          std::find(d->advice_queries.begin(), d->advice_queries.end(), std::make_pair(col, (int32_t)0)) == d->advice_queries.end())
        d->advice_queries.push_back({col, 0});
    }
    off += w;
    d->lookups.push_back(lk);
  }
  if (pl && pk_describe_plonk(cs, off, from_stream, lim, d, err) != CQ_OK) return CQ_ERR_ARG;
  // blinding_factors (plonk/circuit.rs:2022-2047)
  if (pl && pl->blinding_factors) {
    d->bf = pl->blinding_factors;
  } else {
    std::vector<uint32_t> per_col(cs->num_advice, 0);
    for (auto& q : d->advice_queries) per_col[q.first]++;
    uint32_t factors = 1;
    for (uint32_t v : per_col) factors = std::max(factors, v);
    d->bf = std::max(3u, factors) + 2;
  }
  if (n < (size_t)d->bf + 3) return fail("pk: not enough rows available");  // minimum_rows (circuit.rs:2051-2059)
  d->u = (uint32_t)(n - (d->bf + 1));
  if (pl && pl->perm_mapping && !from_stream) {  // Assembly::mapping, read by keygen alone
    const size_t PC = d->perm_columns.size();
    for (size_t cell = 0; cell < PC * n; cell++)
      if (pl->perm_mapping[2 * cell] >= PC || pl->perm_mapping[2 * cell + 1] >= n) return fail("pk: permutation mapping out of range");
  }
  return CQ_OK;
}

}  // namespace cq

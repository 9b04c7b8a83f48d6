// Stand-alone host program for tests/test_sanitizers_cpu.py: the host half of proving-key construction (csrc/pk.hpp:
// pk_describe, pack_programs, pk_pack_programs) over one good description and the bad ones of tests/test_pk_build_gpu.py,
// built with -fsanitize=address,undefined.  Every array is a heap block of exactly its length, so a read past an end is an
// AddressSanitizer report.  The two functions pk.hpp takes from the rest of the library have stand-ins here.
//   pk_describe_check   prints one line for the good description, one per refused one and "ok" (the descriptions at the
//                       accepted limits print nothing); a wrong code, text, field or offset is exit status 1
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include "../../sha2_on_cq_halo2_amd/csrc/pk.hpp"

struct cq_static_table {
  size_t rows;
};
size_t cq::static_table_rows(const cq_static_table* t) { return t->rows; }
// refuses opcode 0xEE, as the interpreter's checker (plonk.hip) refuses every opcode it does not know
bool cq::gate_program_check(const uint32_t* lens, const uint32_t* words, uint32_t num_polys, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t,
                            const char** why, size_t* total_words) {
  size_t off = 0;
  for (uint32_t p = 0; p < num_polys; off += lens[p++])
    for (uint32_t q = 0; q < lens[p]; q++)
      if ((words[off + q] & 0xffu) == 0xEE) {
        *why = "gate program: unknown opcode";
        return false;
      }
  *total_words = off;
  return true;
}

namespace {
constexpr uint32_t K = 5, N = 1u << K, ADVICE = 3, FIXED = 2, PERM = 3;
const cq::PkLimits LIMITS{16, 8, 64, 16};

// a description with everything in it: an expression-valued vector lookup, gates, a legacy lookup, a permutation
struct Description {
  cq_static_table table{16};
  size_t table_rows = 16;
  std::vector<uint32_t> widths{2}, lookup_columns{0, 0};
  std::vector<cq_static_table*> tables{&table, &table};
  std::vector<uint32_t> advice_q{0, 1, 2, 0}, fixed_q{0, 1}, gate_lens{3, 2}, gate_words{1, 0, 5, 2, 0}, perm_kinds{CQ_COL_ADVICE, CQ_COL_FIXED, CQ_COL_INSTANCE},
      perm_idx{2, 1, 0}, lk_lens{2, 4}, lk_words{1, 0, 1, 0, 1, 0}, legacy_widths{2}, legacy_lens{1, 2, 3, 1}, legacy_words{0, 0, 0, 0, 0, 0, 0};
  std::vector<int32_t> advice_r{0, 0, 0, 1}, fixed_r{0, -1};
  std::vector<uint64_t> constants{1, 0, 0, 0};
  std::vector<uint32_t> mapping;
  std::vector<const uint64_t*> fixed{nullptr, nullptr};
  cq_plonk pl{};
  cq_circuit cs{};
  Description() {
    identity_mapping(PERM);
    fixed[0] = fixed[1] = constants.data();  // only their presence is looked at
    pl.cs_degree = 5;
    link();
  }
  void identity_mapping(uint32_t columns) {
    mapping.clear();
    for (uint32_t c = 0; c < columns; c++)
      for (uint32_t r = 0; r < N; r++) {
        mapping.push_back(c);
        mapping.push_back(r);
      }
  }
  void link() {  // after a vector was replaced
    pl.num_fixed = FIXED;
    pl.num_instance = 1;
    pl.fixed = fixed.data();
    pl.num_advice_queries = (uint32_t)advice_q.size();
    pl.advice_query_columns = advice_q.data();
    pl.advice_query_rotations = advice_r.data();
    pl.num_fixed_queries = (uint32_t)fixed_q.size();
    pl.fixed_query_columns = fixed_q.data();
    pl.fixed_query_rotations = fixed_r.data();
    pl.num_gate_polys = (uint32_t)gate_lens.size();
    pl.gate_program_lens = gate_lens.data();
    pl.gate_programs = gate_words.data();
    pl.num_constants = 1;
    pl.constants = constants.data();
    pl.num_perm_columns = (uint32_t)perm_kinds.size();
    pl.perm_column_kinds = perm_kinds.data();
    pl.perm_column_indices = perm_idx.data();
    pl.perm_mapping = mapping.data();
    pl.lookup_input_program_lens = lk_lens.data();
    pl.lookup_input_programs = lk_words.data();
    pl.num_legacy_lookups = 1;
    pl.legacy_lookup_widths = legacy_widths.data();
    pl.legacy_program_lens = legacy_lens.data();
    pl.legacy_programs = legacy_words.data();
    cs.k = K;
    cs.num_advice = ADVICE;
    cs.num_lookups = 1;
    cs.lookup_widths = widths.data();
    cs.lookup_columns = lookup_columns.data();
    cs.lookup_tables = tables.data();
    cs.plonk = &pl;
  }
};

int failures = 0;
void expect(bool cond, const char* what) {
  if (!cond) {
    printf("FAILED: %s\n", what);
    failures++;
  }
}

// describes `d` as pk.hip's driver does and expects CQ_ERR_ARG with exactly `text`
void rejected(const char* text, const std::function<void(Description&)>& spoil, uint32_t params_k = K, bool have_cfg = true, bool have_b0 = true) {
  Description d;
  spoil(d);
  d.link();
  cq_pk_desc desc;
  std::string err;
  const int rc = cq::pk_describe(&d.cs, params_k, have_cfg ? &d.table_rows : nullptr, have_b0, false, LIMITS, &desc, &err);
  printf("%d %s\n", rc, err.c_str());
  expect(rc == CQ_ERR_ARG && err == text, text);
}

// describes `d` after `shape`, as pk.hip's driver does, and expects CQ_OK and `holds`; prints nothing
void accepted(const char* what, const std::function<void(Description&)>& shape, const std::function<bool(Description&, cq_pk_desc&)>& holds) {
  Description d;
  shape(d);
  d.link();
  cq_pk_desc desc;
  std::string err;
  const int rc = cq::pk_describe(&d.cs, K, &d.table_rows, true, false, LIMITS, &desc, &err);
  expect(rc == CQ_OK && err.empty() && holds(d, desc), what);
}
}  // namespace

int main() {
  {  // the good one: fields, then the blobs and their offsets
    Description d;
    cq_pk_desc desc;
    std::string err;
    const int rc = cq::pk_describe(&d.cs, K, &d.table_rows, true, false, LIMITS, &desc, &err);
    printf("%d %s\n", rc, err.c_str());
    expect(rc == CQ_OK && err.empty(), "good description");
    expect(desc.k == K && desc.num_advice == ADVICE && desc.num_fixed == FIXED && desc.num_instance == 1 && desc.cs_degree == 5, "shape");
    expect(desc.bf == 5 && desc.u == N - 6, "blinding factors from the advice queries (column 0 twice), usable rows");
    expect(desc.advice_queries.size() == 4 && desc.advice_queries[3] == std::make_pair(0u, (int32_t)1), "advice queries");
    expect(desc.fixed_queries.size() == 2 && desc.fixed_queries[1] == std::make_pair(1u, (int32_t)-1), "fixed queries");
    expect(desc.perm_columns.size() == PERM && desc.perm_columns[1] == std::make_pair(CQ_COL_FIXED, 1u) && desc.perm_sets() == 1, "permutation columns");
    expect(desc.num_gate_polys == 2 && desc.lookup_exprs && desc.legacy.size() == 1 && desc.legacy[0].width == 2 && desc.general(), "programs");
    expect(desc.lookups.size() == 1 && desc.lookups[0].cols.size() == 2 && desc.lookups[0].tables[1] == &d.table && desc.num_phases == 1, "lookups");
    const cq::PkPrograms prog = cq::pk_pack_programs(&d.pl, &desc);
    expect(prog.gates == std::vector<uint32_t>({3, 1, 0, 5, 2, 2, 0}), "gate blob");
    expect(prog.legacy == std::vector<uint32_t>({1, 0, 2, 0, 0, 3, 0, 0, 0, 1, 0}), "legacy blob");
    expect(desc.legacy[0].in_off == 0 && desc.legacy[0].tab_off == 5, "legacy offsets: inputs at 0, tables behind the two input programs");
    expect(prog.lookups == std::vector<uint32_t>({2, 1, 0, 4, 1, 0, 1, 0}), "lookup input blob");
    expect(desc.lookups[0].prog == std::vector<int64_t>({0, 3}), "lookup input offsets");
    std::vector<size_t> at;
    expect(cq::pack_programs(nullptr, nullptr, 0, &at).empty() && at.empty(), "no programs");
    // from a stream neither the fixed columns nor the mapping are read
    d.pl.fixed = nullptr;
    d.pl.perm_mapping = nullptr;
    cq_pk_desc again;
    expect(cq::pk_describe(&d.cs, K, &d.table_rows, true, true, LIMITS, &again, &err) == CQ_OK, "description of a serialized key");
  }
  // the limits themselves are accepted: degree 3 and 18, 64 permutation columns, a legacy lookup 64 expressions wide
  accepted("cs_degree 18", [](Description& d) { d.pl.cs_degree = 18; }, [](Description&, cq_pk_desc& desc) { return desc.cs_degree == 18 && desc.perm_sets() == 1; });
  accepted("cs_degree 3", [](Description& d) { d.pl.cs_degree = 3; }, [](Description&, cq_pk_desc& desc) { return desc.cs_degree == 3 && desc.perm_sets() == PERM; });
  const auto columns64 = [](Description& d) {
    d.perm_kinds.clear();
    d.perm_idx.clear();
    for (uint32_t c = 0; c < 64; c++) {
      d.perm_kinds.push_back(c % 3 == 2 ? CQ_COL_FIXED : CQ_COL_ADVICE);
      d.perm_idx.push_back(c % 2);
    }
    d.identity_mapping(64);
  };
  accepted("64 permutation columns", columns64, [](Description&, cq_pk_desc& desc) {
    return desc.perm_columns.size() == 64 && desc.perm_sets() == 22 && desc.perm_columns[63] == std::make_pair(CQ_COL_ADVICE, 1u);
  });
  accepted("64 permutation columns, one per set", [&](Description& d) { columns64(d); d.pl.cs_degree = 3; },
           [](Description&, cq_pk_desc& desc) { return desc.perm_sets() == 64; });
  accepted("legacy lookup 64 wide", [](Description& d) { d.legacy_widths[0] = 64; d.legacy_lens.assign(128, 1); d.legacy_words.assign(128, 0); },
           [](Description& d, cq_pk_desc& desc) {
             const cq::PkPrograms prog = cq::pk_pack_programs(&d.pl, &desc);
             return desc.legacy.size() == 1 && desc.legacy[0].width == 64 && prog.legacy.size() == 256 && desc.legacy[0].in_off == 0 &&
                    desc.legacy[0].tab_off == 128;
           });
  {  // opening points: rotations of one residue modulo 2^k are one point
    cq_pk_desc desc;
    desc.k = K;
    const int32_t rots[][2] = {{0, 0}, {1, 1}, {-1, -1}, {15, 15}, {16, -16}, {-16, -16}, {17, -15}, {31, -1}, {-31, 1}, {32, 0}, {-33, -1}, {-6, -6}};
    for (auto& r : rots) expect(desc.point_rotation(r[0]) == r[1], "point_rotation, k = 5");
    desc.k = 3;
    expect(desc.point_rotation(-6) == 2 && desc.point_rotation(4) == -4 && desc.point_rotation(3) == 3, "point_rotation, k = 3");
    desc.k = 0;
    expect(desc.point_rotation(5) == 0 && desc.point_rotation(-1) == 0, "point_rotation, k = 0");
    desc.k = K;
    desc.bf = 5;
    desc.advice_queries = {{0, 0}, {1, -31}, {2, 16}, {0, -16}, {1, 1}};
    desc.fixed_queries = {{0, 31}};
    expect(desc.opening_rotations() == std::vector<int32_t>({0, 1, -16, -1}), "opening rotations without a permutation");
    desc.perm_columns = {{CQ_COL_ADVICE, 0}, {CQ_COL_ADVICE, 1}};  // two sets at degree 3: x, omega x, omega^-6 x
    expect(desc.opening_rotations() == std::vector<int32_t>({0, 1, -16, -1, -6}), "opening rotations with two product sets");
  }
  rejected("pk: circuit k differs from params k", [](Description&) {}, K + 1);
  rejected("pk: static lookups need a table config and b0_g1_bound", [](Description&) {}, K, false, true);
  rejected("pk: static lookups need a table config and b0_g1_bound", [](Description&) {}, K, true, false);
  rejected("pk: table size differs from the table config", [](Description& d) { d.table.rows = 32; });
  rejected("pk: lookup width out of range", [](Description& d) { d.widths[0] = 9; });
  rejected("pk: advice query column out of range", [](Description& d) { d.advice_q[3] = ADVICE; });
  rejected("pk: fixed query column out of range", [](Description& d) { d.fixed_q[1] = FIXED; });
  rejected("pk: permutation column out of range", [](Description& d) { d.perm_idx[0] = ADVICE; });
  rejected("pk: permutation column out of range", [](Description& d) { d.perm_kinds[2] = 3; });
  rejected("pk: permutation mapping out of range", [](Description& d) { d.mapping[2 * (N + 7) + 1] = N; });
  rejected("pk: permutation mapping out of range", [](Description& d) { d.mapping[2 * (PERM * N - 1)] = PERM; });
  rejected("pk: not enough rows available", [](Description& d) { d.pl.blinding_factors = N - 2; });
  rejected("pk: cs_degree out of range", [](Description& d) { d.pl.cs_degree = 19; });
  rejected("gate program: unknown opcode", [](Description& d) { d.gate_words[4] = 0xEE; });
  rejected("gate program: unknown opcode", [](Description& d) { d.legacy_words[6] = 0xEE; });
  rejected("gate program: unknown opcode", [](Description& d) { d.lk_words[5] = 0xEE; });
  rejected("pk: legacy lookup width out of range", [](Description& d) { d.legacy_widths[0] = 65; });
  if (failures) return 1;
  printf("ok\n");
  return 0;
}

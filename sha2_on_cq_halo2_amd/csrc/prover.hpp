// Internal interface of the host orchestrator (prover.hip).
#pragma once
#include <stdint.h>
#include <vector>
#include "../../include/cq_halo2.h"
#include "field.hpp"

struct cq_pk;

namespace cq {
size_t prover_arena_elems(const cq_pk* pk);
int create_proof_dev(cq_pk* pk, const uint64_t* const* advice_dev, const uint64_t* const* instances,
                     const size_t* instance_lens, cq_phase_fn phase_fn, void* phase_user, cq_rng_next_u64 rng_next,
                     void* rng_state, std::vector<uint8_t>& proof_out);
// Single stages of the proof for a caller that keeps its own create_proof: the code create_proof_dev runs for the same
// stage, on caller-owned buffers (cq_permutation_commit_dev, cq_lookup_commit_product_dev, cq_evaluate_h_dev,
// cq_multiopen_dev in capi_rounds.hip, which checks the arguments; shapes in cq_halo2.h).
int stage_permutation_commit(cq_pk* pk, const uint64_t* const* advice_dev, const uint64_t* const* instance_dev, const Fr& beta,
                             const Fr& gamma, cq_rng_next_u64 rng_next, void* rng_state, Fr* z, uint64_t* commitments);
int stage_lookup_commit_product(cq_pk* pk, const uint64_t* const* input_dev, const uint64_t* const* table_dev,
                                const uint64_t* const* permuted_input_dev, const uint64_t* const* permuted_table_dev, const Fr& beta,
                                const Fr& gamma, cq_rng_next_u64 rng_next, void* rng_state, Fr* z, uint64_t* commitments);
int stage_evaluate_h(cq_pk* pk, const uint64_t* const* advice_coeff_dev, const uint64_t* const* instance_coeff_dev, const Fr* perm_z,
                     const uint64_t* const* permuted_input_coeff_dev, const uint64_t* const* permuted_table_coeff_dev, const Fr* lookup_z,
                     const uint64_t* challenges, const Fr& beta, const Fr& gamma, const Fr& theta, const Fr& y, Fr* h_out);
int stage_multiopen(cq_pk* pk, const cq_open_query* queries, size_t count, const cq_open_transcript* transcript);
}  // namespace cq

// Internal interface of the G2 kernels (msm_g2.hip): the multi-scalar multiplication and the fixed-base powers of the
// test SRS.  The G1 engine (msm.hpp) is not involved.
#pragma once
#include <hip/hip_runtime.h>
#include "curve2.hpp"

struct cq_ctx;

namespace cq {

// window width of an n-term G2 MSM (signed digits, 2^(c-1) buckets per window)
uint32_t g2_msm_window_bits(size_t n);
// sum_i scalars[i] * bases[i] over device arrays (Montgomery scalars, reference-layout affine bases); the Jacobian result
// on the host once the stream has drained
int g2_msm(cq_ctx* c, const Fr* scalars_dev, const G2Affine* bases_dev, size_t n, G2Jac* out);
// out[i] = [s^i]_2 for i < count, affine (device)
int g2_srs_powers(cq_ctx* c, const Fr& s, uint32_t count, G2Affine* out_dev);

}  // namespace cq

// SerdeFormat::Processed conversions on the device (serde.hip): compressed G1 / G2 points and canonical scalars <-> the raw
// Montgomery layouts every other entry point takes.
#pragma once
#include "curve.hpp"
#include "curve2.hpp"

struct cq_ctx;

namespace cq {

// Verdict words of the checking conversions, in device memory: *count_dev += the number of invalid elements (atomicAdd),
// *first_dev = min(*first_dev, lowest invalid index) (atomicMin).  serde_verdict_reset sets `cells` of each to 0 / 0xffffffff.
int serde_verdict_reset(cq_ctx* c, uint32_t* count_dev, uint32_t* first_dev, size_t cells);
// `CurveAffine::from_bytes` (derive/curve.rs:603-627): n x 32 B compressed -> n raw affine points.  `in` 16-byte aligned.
int g1_decompress(cq_ctx* c, const uint8_t* in, uint32_t n, G1Affine* out, uint32_t* count_dev, uint32_t* first_dev);
// `CurveAffine::to_bytes` (derive/curve.rs:635-646): n raw affine points -> n x 32 B.  `out` 16-byte aligned.
int g1_compress(cq_ctx* c, const G1Affine* in, uint32_t n, uint8_t* out);
// `Fr::from_repr` / `to_repr` (helpers.rs:68-91): n x 32 B canonical little-endian <-> Montgomery words; `out` may be `in`.
int fr_from_repr(cq_ctx* c, const uint8_t* in, uint32_t n, Fr* out, uint32_t* count_dev, uint32_t* first_dev);
int fr_to_repr(cq_ctx* c, const Fr* in, uint32_t n, uint8_t* out);
// `GroupEncoding::from_bytes` / `to_bytes` for G2Affine (derive/curve.rs:603-646, compressed size 64): n x 64 B compressed
// <-> n raw affine points (x.c0 | x.c1 | y.c0 | y.c1).  Invalid points are reported as index `base` + i.  16-byte aligned.
int g2_decompress(cq_ctx* c, const uint8_t* in, uint32_t n, uint32_t base, G2Affine* out, uint32_t* count_dev, uint32_t* first_dev);
int g2_compress(cq_ctx* c, const G2Affine* in, uint32_t n, uint8_t* out);
// SerdeFormat::RawBytes for G2Affine (derive/curve.rs:649-700): coordinates below q, on the twist or the identity; same verdict
// words, index `base` + i.
int g2_validate(cq_ctx* c, const G2Affine* pts, uint32_t n, uint32_t base, uint32_t* count_dev, uint32_t* first_dev);

}  // namespace cq

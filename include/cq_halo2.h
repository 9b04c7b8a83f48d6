/*
 * cq_halo2.h -- C ABI of the MI355X (gfx950) backend for the CQ-lookup / KZG
 * polynomial-commitment hot path of halo2_proofs::plonk::create_proof.
 *
 * The reference (aleph-zero-foundation/sha2-on-cq-halo2) is 100 % Rust and has no FFI
 * seam; each entry point below replaces one Rust function that `create_proof` and its
 * sub-arguments call (cited as file:line under halo2_proofs/src unless noted).  The Rust
 * binding a maintainer would add is sketched in INTEGRATION.md.
 *
 * Conventions
 *  - Field elements: 4 x uint64_t little-endian limbs of a*2^256 mod p (Montgomery form),
 *    byte-identical to halo2curves `Fr([u64;4])` / `Fq([u64;4])` (arithmetic/curves/src/bn256/fr.rs:25).
 *  - G1 affine: 8 x uint64_t = x || y, identity = all zero (derive/curve.rs:453-463).
 *  - G1 Jacobian: 12 x uint64_t = x || y || z, identity z = 0 (derive/curve.rs:696-705).
 *  - Every function returns CQ_OK (0) or a negative status; nothing unwinds or aborts across
 *    the boundary (the Rust side panics on these contract violations: arithmetic.rs:133,184).
 *  - `_dev` entry points take DEVICE pointers (hipMalloc / cq_dev_alloc / a torch tensor's
 *    data_ptr) and run asynchronously on the context's stream; the others take host slices,
 *    like the Rust functions they replace, and return after the result is in host memory.
 *  - A context is bound to one GPU and one HIP stream and may be used by one thread at a
 *    time (create_proof calls these serially, plonk/prover.rs:51-779); use one context per
 *    thread / per rank for concurrency.
 */
#ifndef CQ_HALO2_H
#define CQ_HALO2_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CQ_OK 0
#define CQ_ERR_ARG (-1)      /* bad argument (length mismatch, not a power of two, null pointer) */
#define CQ_ERR_HIP (-2)      /* HIP runtime failure; see cq_last_error */
#define CQ_ERR_NO_DEVICE (-3)
#define CQ_ERR_LOOKUP (-4)   /* CQ: witness value not in table / vector lookup on different rows */
#define CQ_ERR_INTERNAL (-5)
#define CQ_ERR_TRANSCRIPT (-6) /* a commitment was the identity (transcript.rs:221-227) */

typedef struct cq_ctx cq_ctx;
typedef struct cq_domain cq_domain;   /* EvaluationDomain<Fr>, poly/domain.rs:19-34 */
typedef struct cq_params cq_params;   /* ParamsKZG<Bn256> G1 part, poly/kzg/commitment.rs:31-39 */
typedef struct cq_table_config cq_table_config; /* StaticTableConfig, plonk/static_lookup.rs:47-66 */
typedef struct cq_static_table cq_static_table; /* StaticTableValues, plonk/static_lookup.rs:68-75 */
typedef struct cq_g2_srs cq_g2_srs;   /* the G2 powers of TableSRS, poly/kzg/commitment.rs:73-123 (`g2`) */
typedef struct cq_pk cq_pk;           /* ProvingKey slice read by the CQ-only prover, plonk.rs:291-308 */
/* `R: RngCore` of create_proof (plonk/prover.rs:65): the library calls next_u64 exactly as
 * `Fr::random` does (8 calls per scalar, low limb first, bn256/fr.rs:159-170). */
typedef uint64_t (*cq_rng_next_u64)(void* state);
/* Optional bulk form of the same generator (`RngCore::fill_bytes`): writes the next `count` outputs of next_u64 to
 * dst and advances the state.  See cq_pk_set_rng_fill. */
typedef void (*cq_rng_fill_fn)(void* state, uint64_t* dst, size_t count);
/* Collective hook for MSM sharding (one process per GPU): gathers `bytes_per_rank` bytes from every rank
 * into `recv` (world x bytes_per_rank, rank order).  The host application implements it with RCCL /
 * torch.distributed; returns 0 on success. */
typedef int (*cq_allgather_fn)(void* user, const void* send, void* recv, size_t bytes_per_rank);
/* Broadcast hook for column sharding: `buf` (host memory, `bytes` long) holds the payload on rank `root` and receives it
 * on the others; returns 0 on success. */
typedef int (*cq_bcast_fn)(void* user, void* buf, size_t bytes, uint32_t root);

/* Point-to-point hook for resident column sharding (cq_pk_set_resident_sharding): `count` transfers of HOST buffers
 * between this rank and `peer`, `send` != 0 for outgoing ones.  Every rank is called with its part of one global list, in
 * the same relative order, so the k-th send from a to b meets the k-th receive of b from a.  Returns 0 on success. */
typedef struct { uint32_t peer; uint32_t send; void* buf; size_t bytes; } cq_xfer;
typedef int (*cq_exchange_fn)(void* user, const cq_xfer* xfers, size_t count);

/* ---- context ------------------------------------------------------------------------- */
/* `hip_stream` may be NULL (the library creates its own stream) or an existing hipStream_t
 * (e.g. torch.cuda.current_stream().cuda_stream) that all work is then enqueued on. */
int cq_ctx_create(int device, void* hip_stream, cq_ctx** out);
void cq_ctx_destroy(cq_ctx* ctx);
const char* cq_last_error(const cq_ctx* ctx);
int cq_ctx_sync(cq_ctx* ctx);
/* hipGraph replay of the MSM pipeline (BASELINE configs[4]: "hipGraph-captured rounds"): with `on` != 0 the kernel
 * sequences before and after the accumulate kernel of every MSM launch (sort + plan: ~12 launches; combine + bucket
 * reduction: ~6) are captured once per launch shape and replayed with one hipGraphLaunch each.  Same results; off by
 * default because on ROCm 7.2 it measured no faster than the plain launches.  This is SEGMENT capture: a whole
 * Fiat-Shamir round cannot be one graph here, because a round ends in a host step the next round's kernels depend on --
 * the commitments are normalised and absorbed by the Blake2b transcript on the host and the challenge comes back as a
 * kernel argument -- and the measured idle time between rounds is that host step (fold, normalise, hash: 60-100 us per
 * round, profiles/r03_host_trace_k18.txt), not launch overhead. */
int cq_ctx_set_hip_graphs(cq_ctx* ctx, int on);
/* RCCL communicator of the context (one process per GPU, xGMI within a node): rank 0 draws an id with
 * cq_rccl_unique_id and hands it to the other ranks by whatever means the application has (a torch.distributed
 * broadcast, MPI, a file); every rank then calls cq_ctx_comm_init_rccl -- collectively, it blocks until all have.  The
 * library loads librccl at run time (the copy already in the process, e.g. PyTorch's, else ROCm's) and issues its
 * collectives on the context's stream, on device buffers.  CQ_ERR_NO_DEVICE when librccl cannot be loaded. */
#define CQ_RCCL_UNIQUE_ID_BYTES 128
int cq_rccl_unique_id(uint8_t id[CQ_RCCL_UNIQUE_ID_BYTES]);
int cq_ctx_comm_init_rccl(cq_ctx* ctx, uint32_t rank, uint32_t world, const uint8_t id[CQ_RCCL_UNIQUE_ID_BYTES]);
int cq_ctx_comm_destroy(cq_ctx* ctx);
/* Collective self-check of the communicator, issued the way the sharded prover issues its exchanges: an ncclAllGather
 * on the context's stream; a grouped launch of ncclBroadcasts (one root per rank, unequal lengths of about 1 MiB) on the
 * context's SIDE stream, ordered behind an event of the main stream; a second ncclAllGather on the main stream while the
 * broadcasts are in flight; device buffers, patterns every rank verifies.  Every rank calls it.
 *
 * Failure behaviour of the RCCL transport: the staging its small exchanges need is allocated by cq_ctx_comm_init_rccl, not
 * inside proofs; a sharded proof first agrees that every rank could set itself up (one status word per rank) and returns an
 * error everywhere if one could not; host waits inside a proof poll the stream with a time-out (CQ_COMM_TIMEOUT_S, default
 * 300 s, 0 = none) and ncclCommGetAsyncError; a rank that fails alone in the middle of a proof (CQ_ERR_HIP / _INTERNAL)
 * aborts its communicator (ncclCommAbort) so that its peers fail -- asynchronous error or time-out -- instead of hanging.
 * After an abort the context needs a new communicator (cq_ctx_comm_init_rccl). */
int cq_ctx_comm_selftest(cq_ctx* ctx);
void* cq_ctx_stream(cq_ctx* ctx);
const char* cq_version(void);

/* ---- device memory (plumbing) ------------------------------------------------------------ */
int cq_dev_alloc(cq_ctx* ctx, size_t bytes, void** dptr);
int cq_dev_free(cq_ctx* ctx, void* dptr);
int cq_dev_upload(cq_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int cq_dev_download(cq_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int cq_dev_memset(cq_ctx* ctx, void* dptr, int value, size_t bytes);

/* ---- arithmetic.rs ------------------------------------------------------------------- */
/* best_fft(a, omega, log_n)  arithmetic.rs:171-234.  In place on a host slice of 2^log_n Fr,
 * natural order in and out. */
int cq_best_fft(cq_ctx* ctx, uint64_t* a, uint32_t log_n, const uint64_t omega[4]);
/* Same on device memory; both 2^log_n elements; `out` may alias `in`. */
int cq_best_fft_dev(cq_ctx* ctx, const uint64_t* in_dev, uint64_t* out_dev, uint32_t log_n,
                    const uint64_t omega[4]);

/* best_multiexp(coeffs, bases)  arithmetic.rs:132-159.  sum_i coeffs[i] * bases[i] as a Jacobian
 * point (the caller normalises, e.g. batch_normalize at plonk/prover.rs:363).  `len` is the common
 * length of both slices (the Rust function asserts equality, arithmetic.rs:133). */
int cq_best_multiexp(cq_ctx* ctx, const uint64_t* coeffs, const uint64_t* bases, size_t len,
                     uint64_t out_jac[12]);
/* Same with scalars and bases resident in device memory; the result is written to HOST memory
 * (96 bytes) after the stream has drained. */
int cq_best_multiexp_dev(cq_ctx* ctx, const uint64_t* coeffs_dev, const uint64_t* bases_dev, size_t len,
                         uint64_t out_jac[12]);
/* `count` multiexps over the same bases (e.g. all advice columns of a phase,
 * plonk/prover.rs:356-360): `coeffs_dev` is a HOST array of `count` device pointers; one host
 * synchronisation for the whole batch; out_jac = count x 12 limbs on the host. */
int cq_msm_batch_dev(cq_ctx* ctx, const uint64_t* const* coeffs_dev, const uint64_t* bases_dev, size_t len,
                     size_t count, uint64_t* out_jac);
/* Host helpers for multi-GPU MSM sharding: sum of `count` Jacobian points (the per-rank partial
 * results after an all-gather; EC addition is not an RCCL reduction op), and Curve::to_affine
 * (derive/curve.rs:399-412). */
int cq_g1_sum(const uint64_t* jac_points, size_t count, uint64_t out_jac[12]);
int cq_g1_to_affine(const uint64_t jac[12], uint64_t out_affine[8]);
/* best_multiexp(coeffs, bases) over G2Affine  arithmetic.rs:132-159.  G2 affine points are 16 limbs (x.c0, x.c1, y.c0,
 * y.c1, each 4 Montgomery limbs: halo2curves' SerdeObject raw layout; all zero = identity); the result is Jacobian,
 * 24 limbs (x, y, z; z = 0 = identity) in HOST memory.  Host arrays; the _dev form takes device arrays.  Used for the
 * table commitment of StaticTableValues::commit (static_lookup.rs:141). */
int cq_best_multiexp_g2(cq_ctx* ctx, const uint64_t* coeffs, const uint64_t* bases, size_t len, uint64_t out_jac[24]);
int cq_best_multiexp_g2_dev(cq_ctx* ctx, const uint64_t* coeffs_dev, const uint64_t* bases_dev, size_t len,
                            uint64_t out_jac[24]);
/* The G2 twins of cq_g1_sum / cq_g1_to_affine: sum of `count` Jacobian G2 points, and Curve::to_affine
 * (derive/curve.rs:399-412) on the host. */
int cq_g2_sum(const uint64_t* jac_points, size_t count, uint64_t out_jac[24]);
int cq_g2_to_affine(const uint64_t jac[24], uint64_t out_affine[16]);
/* Fixed-base acceleration: builds per-window tables T[w][i] = 2^(c*w) * bases[i] (ceil(255/c) x n x 64 B of
 * HBM) for a device-resident base array and registers them with the context; later multiexps over
 * that array (or a prefix of it) then need a single bucket set and no window folding.  cq_params_*
 * does this for g and g_lagrange unless disabled with cq_msm_set_precompute(ctx, 0).  Results are
 * identical either way.  The tables are a snapshot of the array: call cq_msm_forget_dev before the array is
 * freed or overwritten (cq_dev_free does it for arrays it frees). */
int cq_msm_precompute_dev(cq_ctx* ctx, const uint64_t* bases_dev, size_t n);
int cq_msm_forget_dev(cq_ctx* ctx, const uint64_t* bases_dev);
int cq_msm_set_precompute(cq_ctx* ctx, int on);
/* Pippenger window width in bits (2..15), 0 = automatic.  Tuning knob; results do not depend on it. */
int cq_msm_set_window(cq_ctx* ctx, uint32_t bits);
/* Window width (8..20) of the per-window tables built from now on by cq_msm_precompute_dev, the params and key
 * constructors; 0 = automatic: every array's own length decides (15 bits up to 2^19 points, 17 from 2^20 on), and a
 * proving key brings the small arrays it multiplies over (table SRS, cached quotients) to the width of its SRS tables --
 * MSMs over different base arrays share a launch only when their tables agree -- whatever was built first on the
 * context.  Tuning knob; results do not depend on it. */
int cq_msm_set_table_window(cq_ctx* ctx, uint32_t bits);
/* Which tables would a multiexp over [bases_dev, bases_dev + n) use?  *bits = their window width, 0 = none (plain
 * Pippenger over the array itself); `preferred_bits` != 0 asks for that width first, as a launch does for the width of
 * its longest MSM.  Introspection for callers and tests: results never depend on it. */
int cq_msm_table_width_dev(cq_ctx* ctx, const uint64_t* bases_dev, size_t n, uint32_t preferred_bits, uint32_t* bits);

/* Sums of base points by bucket -- the launch behind [b_0] and [p] of a proof's round 2, on its own (introspection for
 * callers and tests).  `arrays` base arrays of n affine points each (device) share one index vector index_dev[n] (u32,
 * device): out_dev[a * buckets + b] = the sum of bases_dev[a][i] over the i with index_dev[i] == b, for b < buckets <=
 * 16384, as affine points in the reference's layout -- the identity for a bucket no i names; an index >= buckets names no
 * bucket.  packed == 0: the arrays are in the reference's layout; != 0: in the library's packed form, as
 * cq_pk_b_row_bases_dev returns them.  At most 32 arrays. */
int cq_msm_bucket_sums_dev(cq_ctx* ctx, const uint64_t* const* bases_dev, size_t arrays, int packed, const uint32_t* index_dev, size_t n,
                           size_t buckets, uint64_t* out_dev);

/* eval_polynomial(poly, point)  arithmetic.rs:304-329 */
int cq_eval_polynomial(cq_ctx* ctx, const uint64_t* poly, size_t n, const uint64_t point[4], uint64_t out[4]);
int cq_eval_polynomial_dev(cq_ctx* ctx, const uint64_t* poly_dev, size_t n, const uint64_t point[4], uint64_t out[4]);
/* kate_division(a, b)  arithmetic.rs:351-387: (a(X) - a(b)) / (X - b), n-1 coefficients into q.
 * (The reference's always-on re-multiplication check is a debug assertion and is not reproduced.) */
int cq_kate_division(cq_ctx* ctx, const uint64_t* a, size_t n, const uint64_t b[4], uint64_t* q);
int cq_kate_division_dev(cq_ctx* ctx, const uint64_t* a_dev, size_t n, const uint64_t b[4], uint64_t* q_dev);
/* ff::BatchInvert::batch_invert (ff 0.12; call sites poly.rs:192,232, domain.rs:124,468): in place,
 * zeros stay zero. */
int cq_batch_invert(cq_ctx* ctx, uint64_t* a, size_t n);
int cq_batch_invert_dev(cq_ctx* ctx, uint64_t* a_dev, size_t n);

/* ---- plonk/assigned.rs, poly.rs: Assigned (rational) columns ---------------------------------------- */
/* A column of `Assigned<F>` cells (plonk/assigned.rs:11-18: Zero, Trivial(x), Rational(num, den)) as synthesis leaves it,
 * before batch_invert_assigned (poly.rs:174-241) turns it into field elements.  It crosses as the dense array of
 * `Assigned::numerator` (assigned.rs:281-287) plus the SPARSE list of `Assigned::denominator` (:289-296), which is Some
 * for Rational cells only: "if the denominator is trivial, we can skip it" (poly.rs:189-191, :228-230).  Resolved value
 * of a cell, as `Assigned::evaluate` (assigned.rs:353-366) and the batched form give it:
 *   num                where the row is not listed;
 *   num * den^-1       where the row is listed and den != 0 -- a denominator of one is inverted like any other, as the
 *                      batched path does (evaluate's shortcut for it, :358, gives the same value);
 *   0                  where the row is listed and den == 0 ("x/0 -> 0": ff::BatchInvert leaves zeros at zero). */
typedef struct {
  const uint64_t* num;       /* n elements, Montgomery limbs: Zero -> 0, Trivial(x) -> x, Rational(a, b) -> a */
  const uint32_t* den_rows;  /* den_count rows holding a Rational cell, strictly ascending, each < n */
  const uint64_t* den;       /* den_count denominators, in the order of den_rows; 0 is allowed (x/0 -> 0) */
  size_t den_count;          /* 0 = the column is all Zero / Trivial; den_rows / den may then be NULL */
} cq_assigned_column;
/* batch_invert_assigned / batch_invert_assigned_ref (poly.rs:174-241): `ncols` columns of `n` cells each, all their
 * denominators inverted in one batch.  This is the call keygen makes on `assembly.fixed` (plonk/keygen.rs:244, :320) before
 * the columns go into cq_pk_create, and the one create_proof makes on the advice columns (plonk/prover.rs:337).
 * _dev: every pointer inside `cols` is a DEVICE pointer (the array of structs itself is host memory); out_dev: `ncols`
 * device pointers to n elements each, out_dev[c] may be cols[c].num (in place).  The lists are checked on the GPU; unlike
 * most `_dev` entry points this one returns after the stream has drained (it reads the verdict back).
 * The other form takes host pointers throughout and is staged as cq_batch_invert is; its lists are checked on the host.
 * A list that is not strictly ascending or names a row >= n is CQ_ERR_ARG, cq_last_error names the column and the first
 * offending entry, no output is written and no such row is dereferenced. */
int cq_batch_invert_assigned_dev(cq_ctx* ctx, const cq_assigned_column* cols, size_t ncols, size_t n, uint64_t* const* out_dev);
int cq_batch_invert_assigned(cq_ctx* ctx, const cq_assigned_column* cols, size_t ncols, size_t n, uint64_t* const* out);

/* ---- poly/domain.rs ------------------------------------------------------------------------ */
/* EvaluationDomain::new(j, k)  domain.rs:39-142 */
int cq_domain_create(cq_ctx* ctx, uint32_t j, uint32_t k, cq_domain** out);
void cq_domain_destroy(cq_domain* domain);
uint32_t cq_domain_k(const cq_domain* domain);
uint32_t cq_domain_extended_k(const cq_domain* domain);
/* get_omega / get_omega_inv / get_extended_omega / ifft_divisor (domain.rs:391-410); any pointer may be NULL */
int cq_domain_constants(const cq_domain* domain, uint64_t omega[4], uint64_t omega_inv[4],
                        uint64_t extended_omega[4], uint64_t ifft_divisor[4]);
/* lagrange_to_coeff  domain.rs:238-248 (host slice of n, in place) */
int cq_lagrange_to_coeff(cq_domain* domain, uint64_t* a);
/* coeff_to_extended  domain.rs:252-266 (n coefficients in, 2^extended_k coset evaluations out) */
int cq_coeff_to_extended(cq_domain* domain, const uint64_t* a, uint64_t* out);
/* extended_to_coeff  domain.rs:293-315 (2^extended_k in, n*(j-1) coefficients out) */
int cq_extended_to_coeff(cq_domain* domain, const uint64_t* a, uint64_t* out);
/* Device variants; `batch` columns stored back to back (stride n in, n resp. 2^extended_k out). */
int cq_lagrange_to_coeff_dev(cq_domain* domain, const uint64_t* in_dev, uint64_t* out_dev, uint32_t batch);
int cq_coeff_to_extended_dev(cq_domain* domain, const uint64_t* in_dev, uint64_t* out_dev, uint32_t batch);
int cq_extended_to_coeff_dev(cq_domain* domain, const uint64_t* in_dev, uint64_t* out_dev);

/* ---- poly/kzg/commitment.rs ---------------------------------------------------------------- */
/* ParamsKZG (commitment.rs:31-39): uploads g = [s^i]_1 and g_lagrange = [L_i(s)]_1 (2^k affine
 * points each, host memory, `RawBytes` layout) once; they stay resident in HBM. */
int cq_params_create(cq_ctx* ctx, uint32_t k, const uint64_t* g, const uint64_t* g_lagrange, cq_params** out);
/* ParamsKZG::setup_from_toxic_waste (commitment.rs:209-276; "MUST NOT be used in production"):
 * builds g and g_lagrange on the GPU from the toxic waste `s` -- for tests and benches. */
int cq_params_setup_from_toxic_waste(cq_ctx* ctx, uint32_t k, const uint64_t s[4], cq_params** out);
/* out[i] = scalars[i] * G1::generator(), device in / device out (affine). */
int cq_fixed_base_mul_dev(cq_ctx* ctx, const uint64_t* scalars_dev, size_t n, uint64_t* out_affine_dev);
/* ParamsKZG::read_custom / write_custom in the RawBytes layouts (commitment.rs:366-459):
 * k:u32 LE | n x 64 B g | n x 64 B g_lagrange | 128 B g2 | 128 B s_g2.  read: `checked` != 0 validates
 * every point (SerdeFormat::RawBytes), 0 = RawBytesUnchecked; the G2 tail is ignored.  write: emits the
 * 4 + 128 n byte G1 part.  cq_params_read_full / cq_params_write_full handle the complete stream. */
int cq_params_read_raw(cq_ctx* ctx, const uint8_t* buf, size_t len, int checked, cq_params** out);
int cq_params_write_raw(cq_params* params, uint8_t* buf, size_t cap, size_t* written);
/* SerdeFormat (helpers.rs:8-20), the `format` argument of the readers and writers below. */
#define CQ_SERDE_PROCESSED 0           /* compressed points, canonical scalars: the portable format, half the size */
#define CQ_SERDE_RAW_BYTES 1           /* raw Montgomery limbs, every element validated on read */
#define CQ_SERDE_RAW_BYTES_UNCHECKED 2 /* raw Montgomery limbs, no checks */
/* `CurveAffine::from_bytes` (derive/curve.rs:603-627) for a device array: n x 32 B compressed points (little-endian
 * canonical x, the parity of the canonical y in bit 7 of byte 31, 32 zero bytes = identity) -> n affine points in the raw
 * layout.  One square root in Fq per point, a^((q+1)/4), on the GPU.  An encoding is invalid when x >= q, when x^3 + 3 is
 * not a square, or when x = 0 carries the sign bit: CQ_ERR_ARG, *first_bad (may be NULL) = the LOWEST invalid index, and
 * cq_last_error names it; the output array is then unspecified.  Buffers 16-byte aligned.  Unlike most `_dev` entry points
 * this one returns after the stream has drained (it reads the verdict back). */
int cq_g1_decompress_dev(cq_ctx* ctx, const uint8_t* bytes_dev, size_t n, uint64_t* out_affine_dev, size_t* first_bad);
/* `CurveAffine::to_bytes` (derive/curve.rs:635-646): n raw affine points -> n x 32 B, asynchronous on the context's stream. */
int cq_g1_compress_dev(cq_ctx* ctx, const uint64_t* affine_dev, size_t n, uint8_t* bytes_dev);
/* `SerdePrimeField::read` / `write` with SerdeFormat::Processed (helpers.rs:68-91), i.e. `Fr::from_repr` / `to_repr`: n x 32 B
 * canonical little-endian scalars <-> Montgomery limbs; `out_dev` may be `bytes_dev` (in place).  from_repr rejects values
 * >= r exactly as cq_g1_decompress_dev rejects points (CQ_ERR_ARG, *first_bad, waits for the stream); to_repr is asynchronous. */
int cq_fr_from_repr_dev(cq_ctx* ctx, const uint8_t* bytes_dev, size_t n, uint64_t* out_dev, size_t* first_bad);
int cq_fr_to_repr_dev(cq_ctx* ctx, const uint64_t* in_dev, size_t n, uint8_t* bytes_dev);
/* ParamsKZG::read_custom / write_custom in any SerdeFormat (commitment.rs:366-459).  The raw formats are
 * cq_params_read_raw (checked / unchecked) and cq_params_write_raw.  CQ_SERDE_PROCESSED:
 *   k:u32 LE | n x 32 B g | n x 32 B g_lagrange | [64 B g2 | 64 B s_g2]
 * read: the compressed bytes are staged in device scratch and decompressed on the GPU straight into the resident arrays
 * (the reference decompresses in parallel for the same reason, commitment.rs:394-426); an invalid point is CQ_ERR_ARG and
 * cq_last_error names the array and the index.  As in the raw reader the G2 tail (2 x 64 B compressed here) is ignored on
 * read and not emitted on write, and the params hold none afterwards: cq_params_read_full / cq_params_write_full below are
 * the forms with the tail.  cq_params_serialized_size: the bytes cq_params_write emits (4 + 64 n processed, 4 + 128 n raw;
 * 0 for an unknown format). */
int cq_params_read(cq_ctx* ctx, const uint8_t* buf, size_t len, int format, cq_params** out);
int cq_params_write(cq_params* params, int format, uint8_t* buf, size_t cap, size_t* written);
size_t cq_params_serialized_size(const cq_params* params, int format);
/* `GroupEncoding::from_bytes` for G2Affine (derive/curve.rs:603-627, instantiated at bn256/curve.rs:37-48 with compressed
 * size 64) for a device array: n x 64 B compressed points -> n affine points in the raw layout (x.c0 | x.c1 | y.c0 | y.c1,
 * 16 Montgomery limbs, R = 2^256: `SerdeObject`, derive/curve.rs:649-700).  The encoding is `Fq2::to_bytes` of x
 * (bn256/fq2.rs:134-155: canonical little-endian c0, then c1) with bit 7 of byte 63 set to the parity of the canonical
 * y.c0; 64 zero bytes are the identity.  y = (x^3 + 3/(9+i)).sqrt(), negated when the sign bit differs from the parity
 * of the root's canonical c0 -- `Fq2::sqrt` is Algorithm 9 of eprint 2012/685 (fq2.rs:344-398); the GPU computes the
 * same decoded y with two exponentiations in Fq (csrc/sqrt2_29.hpp), including the one case where the algorithm's choice of
 * root shows: a root with c0 == 0 has parity 0 whichever it is, so from_bytes(to_bytes(P)) is P or -P for such a point
 * depending on the algorithm alone, and that is reproduced.  No subgroup check (the reference has none).  Invalid: c0 >= q,
 * c1 >= q after the sign bit is masked, or x^3 + b' not a square -- which includes x = 0 with the sign bit, b' being a
 * non-square.  Contract otherwise as cq_g1_decompress_dev: CQ_ERR_ARG, *first_bad (may be NULL) = the LOWEST invalid index,
 * cq_last_error names it and the number of invalid points; 16-byte aligned buffers; returns after the stream has drained;
 * n == 0 is CQ_OK. */
int cq_g2_decompress_dev(cq_ctx* ctx, const uint8_t* bytes_dev, size_t n, uint64_t* out_affine_dev, size_t* first_bad);
/* `GroupEncoding::to_bytes` for G2Affine (derive/curve.rs:635-646): n raw affine points -> n x 64 B, asynchronous. */
int cq_g2_compress_dev(cq_ctx* ctx, const uint64_t* affine_dev, size_t n, uint8_t* bytes_dev);
/* ParamsKZG's g2 and s_g2 (commitment.rs:31-39), 16 limbs each in the raw layout, kept in host memory.
 * cq_params_setup_from_toxic_waste stores generator and [s]_2 (commitment.rs:265-266), cq_params_read_full what the stream
 * holds, cq_params_downsize carries them over (commitment.rs:480-492); cq_params_create, cq_params_read and
 * cq_params_read_raw produce params without them.  cq_params_set_g2 stores the caller's two points as given (no check);
 * cq_params_g2 returns CQ_ERR_ARG when the params hold none. */
int cq_params_set_g2(cq_params* params, const uint64_t g2[16], const uint64_t s_g2[16]);
int cq_params_g2(const cq_params* params, uint64_t g2[16], uint64_t s_g2[16]);
/* The complete stream of ParamsKZG::read_custom / write_custom (commitment.rs:366-459) in any CQ_SERDE_* format:
 *   k:u32 LE | n g | n g_lagrange | g2 | s_g2        4 + 64 n + 128 bytes processed, 4 + 128 n + 256 raw
 * read_full: the G1 part as cq_params_read; then the two G2 points are decompressed on the GPU (CQ_SERDE_PROCESSED),
 * validated there -- coordinates below q, on the twist or the identity -- (CQ_SERDE_RAW_BYTES) or copied
 * (CQ_SERDE_RAW_BYTES_UNCHECKED).  An invalid tail point is CQ_ERR_ARG and cq_last_error names `g2` or `s_g2`; so is a
 * buffer shorter than the full size.  write_full: the bytes of cq_params_write followed by the tail; CQ_ERR_ARG when the
 * params hold no tail.  cq_params_serialized_size_full: the bytes write_full emits (0 for NULL or an unknown format). */
int cq_params_read_full(cq_ctx* ctx, const uint8_t* buf, size_t len, int format, cq_params** out);
int cq_params_write_full(cq_params* params, int format, uint8_t* buf, size_t cap, size_t* written);
size_t cq_params_serialized_size_full(const cq_params* params, int format);
/* g_to_lagrange(g, k) (arithmetic.rs:277-301): the Lagrange-basis SRS from the monomial one by an inverse FFT
 * over G1 (device arrays of 2^k affine points). */
int cq_g_to_lagrange_dev(cq_ctx* ctx, const uint64_t* g_dev, uint32_t k, uint64_t* g_lagrange_dev);
/* The same points, the same bytes, by the G1 FFT whose twiddle products are fixed-window chains with wave-uniform control
 * flow (csrc/g1window.hpp) -- the transform behind the trapdoor-free constructors below, for circuit-SRS sizes. */
int cq_g_to_lagrange_windowed_dev(cq_ctx* ctx, const uint64_t* g_dev, uint32_t k, uint64_t* g_lagrange_dev);
/* ParamsKZG from the monomial powers alone -- what a ceremony file holds (commitment.rs:31-39; the reader derives nothing,
 * :383-459, so a deployment that has only g must run g_to_lagrange, arithmetic.rs:277-301, itself).  `g`: 2^k affine points
 * [s^i]_1 in host memory, or in device memory when `g_on_device` != 0 (copied: the caller keeps its array).  g_lagrange is
 * computed on the GPU straight into the resident array.  Window tables are registered and the G2 tail is absent exactly as
 * after cq_params_create. */
int cq_params_from_powers(cq_ctx* ctx, uint32_t k, const uint64_t* g, int g_on_device, cq_params** out);
/* ParamsKZG::downsize(k) (kzg/commitment.rs:480-492): the first 2^k powers and their Lagrange basis (recomputed with
 * g_to_lagrange), as a new object. */
int cq_params_downsize(cq_params* params, uint32_t k, cq_params** out);
void cq_params_destroy(cq_params* params);
const uint64_t* cq_params_g_dev(const cq_params* params);
const uint64_t* cq_params_g_lagrange_dev(const cq_params* params);
/* ParamsKZG::commit (commitment.rs:539-543) / commit_lagrange (:496-504); the blind is ignored by
 * the reference and has no parameter here.  `len` <= 2^k. */
int cq_commit(cq_params* params, const uint64_t* poly, size_t len, uint64_t out_jac[12]);
int cq_commit_lagrange(cq_params* params, const uint64_t* poly, size_t len, uint64_t out_jac[12]);
int cq_commit_dev(cq_params* params, const uint64_t* poly_dev, size_t len, uint64_t out_jac[12]);
int cq_commit_lagrange_dev(cq_params* params, const uint64_t* poly_dev, size_t len, uint64_t out_jac[12]);

/* ---- plonk/static_lookup.rs, plonk/keygen.rs, plonk/prover.rs ------------------------------- */
/* StaticTableConfig::new(size, g1_lagrange, g_lagrange_opening_at_0)  static_lookup.rs:55-65
 * (host arrays of `size` affine points; `size` a power of two). */
int cq_table_config_create(cq_ctx* ctx, size_t size, const uint64_t* g1_lagrange,
                           const uint64_t* g_lagrange_opening_at_0, cq_table_config** out);
/* G1 part of TableSRS::setup_from_toxic_waste (kzg/commitment.rs:73-178), built on the GPU (tests/benches). */
int cq_table_config_setup_from_toxic_waste(cq_ctx* ctx, size_t size, const uint64_t s[4], cq_table_config** out);
/* StaticTableConfig from the first `size` monomial powers, without the trapdoor: the two arrays that
 * TableSRS::setup_from_toxic_waste computes from s (kzg/commitment.rs:125-170) are linear in the powers,
 *   g1_lagrange[i] = [L_i(s)]_1 = (1/N) sum_j w^(-ij) [s^j]_1                                  (commitment.rs:125-153)
 *   g_lagrange_opening_at_0[i] = [(L_i(s) - L_i(0)) / s]_1 = (1/N) sum_(j<N-1) w^(-i(j+1)) [s^j]_1   (commitment.rs:156-170)
 * -- two inverse FFTs over G1 (arithmetic.rs:277-301), the second of the powers moved up by one place.  `srs_g1`: `srs_len`
 * affine points (host, or device when `on_device` != 0) of which the first `size` are used.  CQ_ERR_ARG when `size` is not a
 * power of two, `srs_len < size` or `size > 2^28`.  MSM tables are registered as by cq_table_config_create. */
int cq_table_config_from_srs(cq_ctx* ctx, size_t size, const uint64_t* srs_g1, size_t srs_len, int on_device,
                             cq_table_config** out);
void cq_table_config_destroy(cq_table_config* cfg);
int cq_table_config_download(cq_table_config* cfg, uint64_t* g1_lagrange, uint64_t* g_lagrange_opening_at_0);
/* StaticTableValues {size, value_index_mapping, qs}  static_lookup.rs:68-75.  `values`: `size` unique
 * field elements (CQ_ERR_ARG if not unique, as the assert at :84-85); `qs`: the cached quotient
 * commitments as affine points (normalise the reference's Vec<G1> first). */
int cq_static_table_create(cq_ctx* ctx, size_t size, const uint64_t* values, const uint64_t* qs_affine,
                           cq_static_table** out);
/* Same, with qs computed in closed form from the toxic waste: Q_i = [(T(s)-T(w^i))/(s-w^i) * w^i/N]_1
 * (equal to StaticTableValues::new's O(N^2) result, static_lookup.rs:108-119; tests/benches). */
int cq_static_table_setup_from_toxic_waste(cq_ctx* ctx, size_t size, const uint64_t* values, const uint64_t s[4],
                                           cq_static_table** out);
/* StaticTableValues::new(values, srs_g1) (static_lookup.rs:78-126): the reference's own construction --
 * iNTT of the values, one kate_division + (N-1)-term multiexp per root -- run on the GPU.
 * `srs_g1`: `size` affine powers [s^i]_1 (host). */
int cq_static_table_new(cq_ctx* ctx, size_t size, const uint64_t* values, const uint64_t* srs_g1, cq_static_table** out);
/* Same result as cq_static_table_new (bit-identical qs), computed FK-style ("fast amortized KZG proofs"): one cyclic
 * convolution of size 2N over G1 and one G1 DFT instead of N multiexps -- O(N log N) group operations. */
int cq_static_table_new_fk(cq_ctx* ctx, size_t size, const uint64_t* values, const uint64_t* srs_g1, cq_static_table** out);
/* cq_static_table_new_fk (static_lookup.rs:78-126) with the powers already in device memory, e.g. cq_params_g_dev of params
 * just read: `srs_g1_dev` holds at least `size` affine points and is only read.  `values` stay in host memory. */
int cq_static_table_new_fk_dev(cq_ctx* ctx, size_t size, const uint64_t* values, const uint64_t* srs_g1_dev,
                               cq_static_table** out);
void cq_static_table_destroy(cq_static_table* table);
int cq_static_table_download_qs(cq_static_table* table, uint64_t* qs_affine);
/* The G2 powers of TableSRS (kzg/commitment.rs:73-123, field `g2`): `count` affine points [s^i]_2 resident in HBM.
 * cq_g2_srs_create uploads them from host memory (16 limbs each); with `checked` != 0 every coordinate must be below the
 * modulus and every point on the twist y^2 = x^3 + 3/(9+i) (the identity passes), else CQ_ERR_ARG -- as the
 * RawBytes reads of G1 points.  cq_g2_srs_setup_from_toxic_waste builds [s^i]_2, i < count, on the GPU: the G2 half of
 * TableSRS::setup_from_toxic_waste (tests/benches).  cq_g2_srs_dev: the device array. */
int cq_g2_srs_create(cq_ctx* ctx, size_t count, const uint64_t* points, int checked, cq_g2_srs** out);
int cq_g2_srs_setup_from_toxic_waste(cq_ctx* ctx, size_t count, const uint64_t s[4], cq_g2_srs** out);
int cq_g2_srs_download(cq_g2_srs* srs, uint64_t* points);
size_t cq_g2_srs_len(const cq_g2_srs* srs);
const uint64_t* cq_g2_srs_dev(const cq_g2_srs* srs);
void cq_g2_srs_destroy(cq_g2_srs* srs);
/* The G2 powers as a byte stream.  TableSRS has no serialisation in the reference; the stream is what
 * `for p in srs.g2() { p.write(w, format) }` produces (`SerdeCurveAffine::write`, helpers.rs): `count` points back to back,
 * no header, 64 B each processed / 128 B raw; the count comes from `len`, which must be a multiple of the point size.
 * read: the bytes are staged in device scratch (in chunks) and converted on the GPU -- CQ_SERDE_PROCESSED decompresses as
 * cq_g2_decompress_dev, CQ_SERDE_RAW_BYTES checks every point as cq_g2_srs_create(checked) does but on the GPU,
 * CQ_SERDE_RAW_BYTES_UNCHECKED is one copy.  An invalid point is CQ_ERR_ARG and cq_last_error names its index in the whole
 * array.  write: CQ_ERR_ARG when `cap` is too small.  cq_g2_srs_serialized_size: 0 for NULL or an unknown format. */
int cq_g2_srs_read(cq_ctx* ctx, const uint8_t* buf, size_t len, int format, cq_g2_srs** out);
int cq_g2_srs_write(cq_g2_srs* srs, int format, uint8_t* buf, size_t cap, size_t* written);
size_t cq_g2_srs_serialized_size(const cq_g2_srs* srs, int format);
/* StaticTableValues::commit(srs_g2, srs_g1_len, circuit_n)  static_lookup.rs:128-157: the StaticCommittedTable that
 * keygen_vk stores in vk.static_table_mapping (plonk/keygen.rs:261-265), as three affine G2 points (16 limbs each):
 *   t          = best_multiexp(iNTT(values in ascending canonical order), srs_g2[..N])  -- the reference interpolates
 *                the keys of its value -> index BTreeMap, so the table's own order does not matter;
 *   zv         = srs_g2[N] - srs_g2[0];
 *   x_b0_bound = srs_g2[srs_g1_len - 1 - (circuit_n - 2)].
 * CQ_ERR_ARG (where the reference would panic) when srs_g2 has fewer than N + 1 points, circuit_n < 2, or the
 * x_b0_bound index is negative or past the end of srs_g2. */
int cq_static_table_commit(cq_static_table* table, cq_g2_srs* srs_g2, size_t srs_g1_len, size_t circuit_n, uint64_t zv[16],
                           uint64_t t[16], uint64_t x_b0_bound[16]);

/* Gate polynomials (`Expression`, plonk/circuit.rs:780-1100, as stored in vk.cs.gates after selector
 * compression) cross the boundary as postfix programs of u32 words: word = op | arg << 8.  A column query
 * (arg = column index) is followed by one word holding the rotation as int32.  CONST pushes
 * constants[arg], SCALE multiplies the top of the stack by constants[arg] (Expression::Scaled),
 * NEG/ADD/MUL are Expression::Negated/Sum/Product.  Each program must leave exactly one value. */
#define CQ_GATE_CONST 0u
#define CQ_GATE_ADVICE 1u
#define CQ_GATE_FIXED 2u
#define CQ_GATE_INSTANCE 3u
#define CQ_GATE_NEG 4u
#define CQ_GATE_ADD 5u
#define CQ_GATE_MUL 6u
#define CQ_GATE_SCALE 7u
#define CQ_GATE_CHALLENGE 8u /* pushes user challenge `arg` (Expression::Challenge, circuit.rs:793-794) */
/* column kinds (`Any`, plonk/circuit.rs:141-160) */
#define CQ_COL_ADVICE 0u
#define CQ_COL_FIXED 1u
#define CQ_COL_INSTANCE 2u

/* The part of ConstraintSystem / ProvingKey a general circuit adds to the CQ-only shape: fixed and
 * instance columns, custom gates, the permutation argument.  All host pointers, read during
 * cq_pk_create only. */
typedef struct {
  uint32_t num_fixed;               /* cs.num_fixed_columns (+ compressed selector columns) */
  uint32_t num_instance;            /* cs.num_instance_columns */
  const uint64_t* const* fixed;     /* pk.fixed_values: num_fixed columns of 2^k elements (keygen.rs:320-326) */
  uint32_t cs_degree;               /* vk.cs_degree = cs.degree() (circuit.rs:1979-2018); 0 = 3 */
  uint32_t blinding_factors;        /* cs.blinding_factors() (circuit.rs:2022-2047); 0 = derive from advice queries */
  /* cs.advice_queries / cs.fixed_queries in registration order; evaluations are written in this order
   * (prover.rs:654-687).  When num_advice_queries == 0 the advice queries are derived as for a CQ-only
   * circuit (one query at Rotation::cur() per lookup input, first-seen order). */
  uint32_t num_advice_queries;
  const uint32_t* advice_query_columns;
  const int32_t* advice_query_rotations;
  uint32_t num_fixed_queries;
  const uint32_t* fixed_query_columns;
  const int32_t* fixed_query_rotations;
  /* gate polynomials in cs.gates order (evaluation.rs:226-235) */
  uint32_t num_gate_polys;
  const uint32_t* gate_program_lens;   /* words per polynomial */
  const uint32_t* gate_programs;       /* concatenated */
  uint32_t num_constants;
  const uint64_t* constants;           /* num_constants field elements */
  /* cs.permutation.columns (permutation.rs:20-38) and permutation::keygen::Assembly.mapping
   * (permutation/keygen.rs:14-20): for column position c and row r, mapping[(c * 2^k + r) * 2] =
   * permuted column position, [.. + 1] = permuted row.  NULL mapping = identity (no copy constraints). */
  uint32_t num_perm_columns;
  const uint32_t* perm_column_kinds;   /* CQ_COL_* */
  const uint32_t* perm_column_indices;
  const uint32_t* perm_mapping;
  /* Static lookup inputs as expressions (`Argument::input: Vec<Expression<F>>`, static_lookup.rs:171-178):
   * one postfix program per (lookup, table column) pair in the order of cq_circuit.lookup_columns, sharing
   * `constants`; evaluated over the Lagrange basis as `evaluate(expr, n, 1, ..)` does
   * (static_lookup/prover.rs:91-107).  NULL = every input is advice[lookup_columns[i]] @ Rotation::cur(). */
  const uint32_t* lookup_input_program_lens;
  const uint32_t* lookup_input_programs;
  /* Legacy (plookup-style) lookups, `cs.lookups` (plonk/lookup.rs:9-36): lookup l has legacy_lookup_widths[l] input
   * expressions and as many table expressions; programs are flattened lookup by lookup, inputs first, then tables,
   * and share `constants`.  The grand product, its quotient terms, all commitments and the sort of
   * `permute_expression_pair` (lookup/prover.rs:400-502; cq_permute_expression_pair_dev) run on the GPU. */
  uint32_t num_legacy_lookups;
  const uint32_t* legacy_lookup_widths;
  const uint32_t* legacy_program_lens;
  const uint32_t* legacy_programs;
  /* Phases (circuit.rs `advice_column_phase`, `challenge_phase`; prover.rs:392-464): advice column c is committed in
   * phase advice_column_phases[c] (NULL = everything in the first phase); user challenge i is squeezed after the
   * commitments of phase challenge_phases[i].  Circuits with more than one phase are proven with
   * cq_create_proof_phases. */
  const uint8_t* advice_column_phases;
  uint32_t num_challenges;
  const uint8_t* challenge_phases;
} cq_plonk;

/* Shape of the constraint system (stands in for ConstraintSystem, plonk/circuit.rs):
 * `num_advice` advice columns; lookup l has `lookup_widths[l]` (input, table) pairs; inputs are
 * advice[column] @ Rotation::cur() (lookup_static, circuit.rs:1579-1602), flattened in
 * lookup_columns / lookup_tables.  vk_repr = VerifyingKey::transcript_repr (plonk.rs:221-232).
 * `plonk` = NULL for a CQ-only circuit (advice columns + static lookups). */
typedef struct {
  uint32_t k;
  uint32_t num_advice;
  uint32_t num_lookups;
  const uint32_t* lookup_widths;
  const uint32_t* lookup_columns;
  cq_static_table* const* lookup_tables;
  uint64_t vk_repr[4];
  const cq_plonk* plonk;
} cq_circuit;

/* permutation::keygen::Assembly (permutation/keygen.rs:14-113): the copy-constraint bookkeeping keygen
 * runs while synthesizing; `mapping` (columns * n * 2 words, layout above) starts as the identity from
 * cq_permutation_assembly_init.  cq_permutation_assembly_copy merges the two cells' cycles exactly as
 * Assembly::copy (:43-112); CQ_ERR_ARG on an out-of-range column / row (Error::BoundsFailure).
 * `aux` and `sizes`: caller-provided scratch of columns*n*2 and columns*n words. */
void cq_permutation_assembly_init(uint32_t columns, uint32_t n, uint32_t* mapping, uint32_t* aux, uint32_t* sizes);
int cq_permutation_assembly_copy(uint32_t columns, uint32_t n, uint32_t* mapping, uint32_t* aux, uint32_t* sizes,
                                 uint32_t left_column, uint32_t left_row, uint32_t right_column, uint32_t right_row);
/* keygen_pk (plonk/keygen.rs:278-397): the domain, l0 / l_last / l_active_row on the extended coset
 * (:338-373), fixed polys and cosets (:328-336), the permutation proving key (permutation/keygen.rs:151-208),
 * the table config and `b0_g1_bound` (n-1 affine points; device pointer if b0_on_device != 0, else
 * host; may be NULL when the circuit has no static lookup, as may `cfg`).
 * Lifetimes: `params`, `cfg` and the static tables must outlive the key (as `ProvingKey<'params>` borrows them in the
 * reference); destroy keys first.  (cq_params_destroy / cq_table_config_destroy called while a key still uses the object
 * only mark it released -- the last such key frees it -- so a wrong order leaks nothing and touches no freed memory; the
 * static tables have no such grace.) */
int cq_pk_create(cq_ctx* ctx, cq_params* params, const cq_circuit* circuit, cq_table_config* cfg,
                 const uint64_t* b0_g1_bound, int b0_on_device, cq_pk** out);
/* ProvingKey::write / ProvingKey::read, SerdeFormat::RawBytes / RawBytesUnchecked (plonk.rs:349-403).  Layout:
 *   VerifyingKey::write (:92-113): k:u32 BE | #fixed:u32 BE | fixed commitments (64 B each, raw Montgomery x||y) |
 *     permutation commitments (64 B each) | per selector 2^k/8 bytes of packed bits (helpers.rs:98-105)
 *   then l0 | l_last | l_active_row | fixed_values | fixed_polys | fixed_cosets | permutation {permutations, polys,
 *     cosets} where a polynomial is len:u32 BE + len x 32 B raw limbs (poly.rs:163-170) and a slice of
 *     polynomials starts with its count:u32 BE (helpers.rs:129-140).
 * cq_pk_read_raw = cq_pk_create with those polynomials uploaded straight into HBM instead of recomputed (cosets
 * included: no NTT runs); `circuit` gives the shape (its plonk->fixed / perm_mapping are not read), `num_selectors`
 * the number of selector bit vectors to skip, `checked` != 0 validates every element the key keeps (RawBytes; l0 / l_last of a
 * CQ-only key and the commitments are skipped unread).  The Rust reader
 * leaves static tables / b0_g1_bound empty (:396-401, "FIXME"); here they are passed as for cq_pk_create.
 * cq_pk_write_raw emits the same stream (`selector_bits` is copied through: the prover does not keep selectors). */
int cq_pk_read_raw(cq_ctx* ctx, cq_params* params, const cq_circuit* circuit, cq_table_config* cfg,
                   const uint64_t* b0_g1_bound, int b0_on_device, const uint8_t* buf, size_t len, uint32_t num_selectors,
                   int checked, cq_pk** out);
size_t cq_pk_raw_size(const cq_pk* pk, uint32_t num_selectors);
int cq_pk_write_raw(cq_pk* pk, const uint8_t* selector_bits, uint32_t num_selectors, uint8_t* buf, size_t cap, size_t* written);
/* ProvingKey::read / ProvingKey::write in any SerdeFormat (plonk.rs:349-403): the arguments of the raw trio plus `format`.
 * The raw formats behave as cq_pk_read_raw (checked / unchecked) / cq_pk_write_raw.  CQ_SERDE_PROCESSED is the stream
 * documented above with 32-byte compressed fixed and permutation commitments and 32-byte canonical little-endian scalars in
 * every polynomial; counts, lengths and selector bits are unchanged.  read: the scalars are converted on the GPU where they
 * land and nothing is recomputed (no NTT runs, as for raw); the commitments are decompressed only to validate them.  A scalar
 * >= r anywhere in the stream (sections the prover does not keep included) or an invalid commitment is CQ_ERR_ARG, and cq_last_error names the polynomial (in stream order, l0 = 0) and the
 * element, or the commitment (fixed ones first).  StaticTableValues are not part of the stream (plonk.rs:396-401). */
int cq_pk_read(cq_ctx* ctx, cq_params* params, const cq_circuit* circuit, cq_table_config* cfg, const uint64_t* b0_g1_bound,
               int b0_on_device, const uint8_t* buf, size_t len, uint32_t num_selectors, int format, cq_pk** out);
size_t cq_pk_serialized_size(const cq_pk* pk, int format, uint32_t num_selectors);
int cq_pk_write(cq_pk* pk, int format, const uint8_t* selector_bits, uint32_t num_selectors, uint8_t* buf, size_t cap, size_t* written);
/* Shards every commitment of cq_create_proof across `world` ranks by point range: rank r
 * multiplies the slice shard(len, r, world) of each (scalars, bases) pair, the 96-byte Jacobian partials of a round are
 * all-gathered and summed locally (EC addition is not an RCCL reduction op), so every rank derives the same
 * transcript.  Every rank must hold the same witness and RNG stream.  `fn` = NULL: the exchange is an ncclAllGather
 * on the context's RCCL communicator (cq_ctx_comm_init_rccl with the same rank / world); otherwise the caller's
 * collective on host buffers.  The key's MSM window tables are rebuilt for the rank's slices only (1 / world of the
 * 17 x SRS); world = 1 restores the unsharded key -- except over a one-rank RCCL communicator (fn = NULL), where the
 * prover still issues every collective, over the one rank: the path a single-GPU machine can exercise. */
int cq_pk_set_sharding(cq_pk* pk, uint32_t rank, uint32_t world, cq_allgather_fn fn, void* user);
/* Column sharding, on by default when sharded and a transport for whole columns exists: the independent
 * column transforms of a proof (advice / f / b -> coefficients, -> extended coset: plonk/prover.rs:587-603,
 * evaluation.rs:317-335, static_lookup/prover.rs:271,327) are computed by their owner rank only and broadcast, instead
 * of by every rank.  Transport: RCCL broadcasts on device buffers (`fn` = NULL, needs the context communicator), or the
 * caller's broadcast on host buffers.  `on` = 0 replicates the transforms on every rank. */
int cq_pk_set_column_sharding(cq_pk* pk, int on, cq_bcast_fn fn, void* user);
/* Resident column sharding: the next step after column sharding for the CQ-shaped circuits of the BASELINE configs (advice
 * columns + static lookups on plain advice inputs, one phase, GWC): a transformed column STAYS on its owner -- lookup l's f
 * and b polynomials and their extended cosets on the owner of lookup l, an advice polynomial on the owner of its column --
 * and only what another rank consumes travels, by point range: the slices of b_0 each rank commits (static_lookup/prover.rs:
 * 299,310), the per-owner partial quotients summed slice-wise into the h pieces each rank commits (evaluation.rs:533-548 is
 * a sum over lookups, extended_to_coeff and commit are linear), partial evaluations (a 32-byte sum per query) and the
 * slices of the GWC batch polynomial, whose kate_division runs per range with a carried Horner value.  Per proof and rank
 * that is ~(3 + L / world) x 32 B x 2^k / world x (world - 1) received instead of ~(5 L + A) x 32 B x 2^k broadcast.
 * Same proof bytes.  Transport: grouped ncclSend / ncclRecv on the context's communicator (`fn` = NULL) or the caller's
 * point-to-point hook on host buffers.  Other circuits keep the column-sharding mode set above. */
int cq_pk_set_resident_sharding(cq_pk* pk, int on, cq_exchange_fn fn, void* user);
/* Multi-open scheme of cq_create_proof*: `P: Prover` of create_proof (prover.rs:55).
 * CQ_OPENER_GWC = ProverGWC (poly/kzg/multiopen/gwc/prover.rs:42-91, one witness commitment per distinct
 * point; the default, as in tests/my_test.rs), CQ_OPENER_SHPLONK = ProverSHPLONK
 * (poly/kzg/multiopen/shplonk/prover.rs:120-286, two commitments). */
#define CQ_OPENER_GWC 0
#define CQ_OPENER_SHPLONK 1
int cq_pk_set_opener(cq_pk* pk, int opener);
/* The vanishing argument's random polynomial takes 8 * 2^k words of the caller's RNG (vanishing/prover.rs:51-55): one
 * indirect next_u64 call per word, made on a helper thread of the library while the GPU runs the first rounds.  A
 * caller whose generator can produce words in bulk registers `fill` here (NULL = back to per-word calls); the
 * `rng_state` given to cq_create_proof* is handed to it, and it must yield exactly the words `count` next_u64 calls
 * would.  Either way the callbacks may run on a thread other than the caller's, never concurrently. */
int cq_pk_set_rng_fill(cq_pk* pk, cq_rng_fill_fn fill);
void cq_pk_destroy(cq_pk* pk);
uint32_t cq_pk_usable_rows(const cq_pk* pk);
/* The key's per-row bases of [b_0] (which = 0) and [p] (which = 1): 2^k points in the library's packed form (device), so
 * that [b_0] = sum_i b(w^i) * bases[i]; NULL when the key has none (no static lookups, or a table of more than 16383 rows).
 * Introspection for tests (cq_msm_bucket_sums_dev takes them). */
const uint64_t* cq_pk_b_row_bases_dev(const cq_pk* pk, int which);
size_t cq_pk_proof_size(const cq_pk* pk);
/* create_proof (plonk/prover.rs:51-779) with ProverGWC + Blake2bWrite<Challenge255>.
 * advice_dev: `num_advice` DEVICE pointers to 2^k field elements each; rows [0, usable_rows) are the
 * assigned witness (unassigned cells zero), the rest is ignored (blinding rows are drawn from rng).
 * The proof (cq_pk_proof_size bytes) is written to `proof`. */
int cq_create_proof(cq_pk* pk, const uint64_t* const* advice_dev, cq_rng_next_u64 rng, void* rng_state,
                    uint8_t* proof, size_t proof_cap, size_t* proof_len);
/* `count` independent proofs of the circuit (BASELINE configs[4]: batches of instances): advice_dev[i] = the num_advice
 * device columns of instance i, rng_states[i] its RNG state (one `rng` function for all), proofs[i] / proof_lens[i] its
 * output (proof_cap bytes each).  The proofs are the ones cq_create_proof gives for the same (witness, RNG) one at a
 * time; here up to `lanes` (0 = 3) of them are in flight on the GPU at once, each on a library-owned stream and host
 * thread, so that one proof's latency-bound stretches are filled by another's kernels.  For circuits without instance
 * columns and with a single phase.  (Set GPU_MAX_HW_QUEUES >= 8 in the environment: HIP multiplexes a process's
 * streams onto 4 hardware queues by default and every lane uses three.) */
int cq_create_proof_batch(cq_pk* pk, size_t count, const uint64_t* const* const* advice_dev, cq_rng_next_u64 rng,
                          void* const* rng_states, uint8_t* const* proofs, size_t proof_cap, size_t* proof_lens, uint32_t lanes);
/* Same with host-resident advice columns (uploaded first). */
int cq_create_proof_host(cq_pk* pk, const uint64_t* const* advice, cq_rng_next_u64 rng, void* rng_state,
                         uint8_t* proof, size_t proof_cap, size_t* proof_len);
/* create_proof from the `WitnessCollection` hand-over (plonk/prover.rs:337-360): `cols` = num_advice HOST columns of
 * Assigned cells (2^k rows each), resolved on the GPU by batch_invert_assigned before the blinding rows are drawn
 * (:346-355).  Numerators are uploaded as cq_create_proof_host uploads columns (usable rows only), the sparse
 * denominators next to them, and the proof continues as the host path does.  Listed rows >= usable_rows are ignored: the
 * reference overwrites those cells with blinding (:346-349).  The step draws no randomness: the bytes are those of
 * cq_create_proof_instances on the resolved dense witness with the same RNG stream.  instances / instance_lens as there
 * (NULL without instance columns).  Sharded keys as cq_create_proof_host: every rank resolves its own copy.  CQ_ERR_ARG:
 * a bad row list (as cq_batch_invert_assigned), a multi-phase circuit (cq_create_proof_phases: its callback writes device
 * columns, which cq_batch_invert_assigned_dev resolves). */
int cq_create_proof_assigned(cq_pk* pk, const cq_assigned_column* cols, const uint64_t* const* instances,
                             const size_t* instance_lens, cq_rng_next_u64 rng, void* rng_state, uint8_t* proof,
                             size_t proof_cap, size_t* proof_len);
/* create_proof with public inputs (`instances: &[&[Fr]]`, prover.rs:64): `instances[c]` = HOST pointer to
 * `instance_lens[c]` elements of instance column c (CQ_ERR_ARG if longer than usable_rows: "InstanceTooLarge",
 * :108-110).  ProverGWC has QUERY_INSTANCE = false: the values are absorbed into the transcript (:305-312)
 * and no instance commitment / evaluation is written.  `advice_on_device` selects the two variants above. */
int cq_create_proof_instances(cq_pk* pk, const uint64_t* const* advice, int advice_on_device,
                              const uint64_t* const* instances, const size_t* instance_lens, cq_rng_next_u64 rng,
                              void* rng_state, uint8_t* proof, size_t proof_cap, size_t* proof_len);
/* Multi-phase circuits: the witness of phase p > 0 depends on the challenges squeezed after the commitments of the
 * earlier phases (`WitnessCollection::next_phase`, prover.rs:299-391; the synthesis loop :436-463).  Before it
 * commits the columns of phase p the library calls `phase_fn(user, p, challenges, advice_dev)`: `challenges` holds
 * num_challenges x 4 limbs (those of later phases are zero), and the callback fills the phase-p advice columns
 * (device memory, rows [0, usable_rows)) -- it stands in for re-running `FloorPlanner::synthesize` with
 * `current_phase = p`.  A non-zero return aborts the proof (CQ_ERR_ARG). */
typedef int (*cq_phase_fn)(void* user, uint32_t phase, const uint64_t* challenges, uint64_t* const* advice_dev);
int cq_create_proof_phases(cq_pk* pk, uint64_t* const* advice_dev, const uint64_t* const* instances,
                           const size_t* instance_lens, cq_phase_fn phase_fn, void* phase_user, cq_rng_next_u64 rng,
                           void* rng_state, uint8_t* proof, size_t proof_cap, size_t* proof_len);
/* ---- dev.rs: MockProver::verify on the GPU ---------------------------------------------------------------------------
 * cq_pk_check_witness checks the witness a caller is about to prove against the key, as `MockProver::verify` does
 * (dev.rs:601-958), extended to static lookups (which MockProver ignores, dev.rs:345-350), and says WHICH constraint
 * fails on WHICH row.  A finding is (kind, index, row, detail):
 *   CQ_FAIL_GATE           VerifyFailure::ConstraintNotSatisfied (dev.rs:694-766): index = gate polynomial in cs.gates order
 *                          (the order of cq_plonk.gate_programs), row = the row it was evaluated on.  Every polynomial is
 *                          evaluated on every row 0 .. n-1, blinding rows included, rotations taken mod n.
 *   CQ_FAIL_GATE_POISONED  VerifyFailure::ConstraintPoisoned (dev.rs:755): the polynomial reads an advice cell of a blinding
 *                          row (rows >= usable_rows are poisoned, dev.rs:546-548; the caller's values there are ignored, as
 *                          the prover ignores them) that nothing multiplies by zero.  Poison propagates as `Value` does
 *                          (dev.rs:126-178): -P = P, P + x = P, P * 0 = 0, P * x = P, P scaled by 0 = 0.  Unlike the
 *                          reference, these findings carry their row and are not de-duplicated.
 *   CQ_FAIL_LOOKUP         VerifyFailure::Lookup (dev.rs:768-906): index = legacy lookup, row = a usable row whose tuple of
 *                          input expressions equals the tuple of table expressions on no usable row.  Whole tuples are
 *                          compared (no compression by a challenge); a poisoned entry equals a poisoned entry only
 *                          (`Value` derives Eq, dev.rs:109).
 *   CQ_FAIL_STATIC_LOOKUP  no counterpart in the reference: index = static lookup, row = usable input row, detail =
 *                          0 "not in table" (static_lookup/prover.rs:141) | 1 "Vector lookup must be on the same table row"
 *                          (:148) | 2 the input expression is poisoned on this row (the prover would look up a value it
 *                          draws at random).  The table columns are tried in order and the first objection decides.
 *   CQ_FAIL_PERMUTATION    VerifyFailure::Permutation (dev.rs:908-951): index = position in cs.permutation.columns, row:
 *                          the cell's value differs from the value of the cell the permutation maps it to.  All n rows; a
 *                          copy constraint can only name usable rows (dev.rs:457), so blinding-row cells map to themselves.
 *                          The mapping is recovered from the key's sigma values delta^c' omega^r' (permutation/keygen.rs:
 *                          151-208), so keys made by cq_pk_read_raw are checked like those of cq_pk_create.
 * Fixed and instance cells are never poisoned; instance rows beyond instance_lens[c] are zero.
 *
 * advice: num_advice columns of 2^k elements, all phases (HOST pointers, or DEVICE pointers if advice_on_device != 0);
 * instances / instance_lens as for cq_create_proof_instances; challenges: num_challenges x 4 limbs (HOST), the values the
 * later-phase columns were synthesised with -- no transcript is squeezed; may be NULL when the circuit has none.
 * Returns CQ_OK whenever the check ran: *total = the exact number of findings (it may exceed cap) and
 * failures[0 .. min(cap, *total)) = the first ones in ascending (kind, index, row) order -- the same list on every run, for
 * host or device advice.  cap = 0 with failures = NULL asks only whether the witness is satisfying.  A value missing from
 * a table is a finding, never CQ_ERR_LOOKUP.  CQ_ERR_ARG: an instance column longer than usable_rows, missing instances,
 * NULL challenges for a circuit that has some, a sharded key (cq_pk_set_sharding world > 1).
 * Draws no randomness, writes nothing to the key, and a following cq_create_proof* gives the bytes it would have given
 * without the call. */
#define CQ_FAIL_GATE 1u
#define CQ_FAIL_GATE_POISONED 2u
#define CQ_FAIL_LOOKUP 3u
#define CQ_FAIL_STATIC_LOOKUP 4u
#define CQ_FAIL_PERMUTATION 5u
typedef struct { uint32_t kind; uint32_t index; uint32_t row; uint32_t detail; } cq_witness_failure;
int cq_pk_check_witness(cq_pk* pk, const uint64_t* const* advice, int advice_on_device, const uint64_t* const* instances,
                        const size_t* instance_lens, const uint64_t* challenges, cq_witness_failure* failures, size_t cap,
                        size_t* total);
/* ---- the CQ sub-arguments on their own (for a host that keeps its own create_proof and swaps in only these) ---------
 * Shapes: L = lookups of `pk`, n = 2^k, N = table size, ext = 2^extended_k; lookups in cs.static_lookups order.
 *
 * static_lookup::Argument::commit (plonk/static_lookup/prover.rs:51-183), called at plonk/prover.rs:512-522: evaluates
 * the lookup inputs over the Lagrange basis, compresses them with theta into f (:108-116), maps every usable row to its
 * table index and counts the multiplicities m (:122-160; CQ_ERR_LOOKUP as the reference's errors), commits both.
 *   advice_dev:   num_advice DEVICE columns of n elements, blinding rows included (f is committed over all n rows)
 *   instance_dev: num_instance device columns (NULL without instance columns); challenges: num_challenges x 4 limbs, HOST
 *   f_dev:  L x n elements out (Lagrange values of f);  m_dev: L x N uint32 out (m_sparse, dense)
 *   commitments: HOST, L x 2 affine points (8 limbs each): f_cm, m_cm per lookup -- the order they are written (:175-176) */
int cq_cq_round1_dev(cq_pk* pk, const uint64_t* const* advice_dev, const uint64_t* const* instance_dev, const uint64_t* challenges,
                     const uint64_t theta[4], uint64_t* f_dev, uint32_t* m_dev, uint64_t* commitments);
/* static_lookup::Committed::commit_log_derivatives (:187-342), called at plonk/prover.rs:572-575: A_i = m_i / (t_i + beta)
 * and its three commitments over the table SRS / cached quotients (:224-257), B = 1 / (f + beta), b = iNTT(B) (:261-276),
 * b_0 = (b - b(0)) / X, its commitment and the degree-bound commitment p (:279-313), a(0) (:318-324), f in coefficient
 * form (:326-334).
 *   f_dev, m_dev: as left by cq_cq_round1_dev;  b_coeff_dev, f_coeff_dev: L x n elements out (b_0 is b_coeff + 1, n - 1 long)
 *   commitments: HOST, L x 5 affine points: a, q_a, a_0, b_0, p per lookup (write order :306-313); a_at_zero: HOST, L x 4 limbs */
int cq_cq_round2_dev(cq_pk* pk, const uint64_t* f_dev, const uint32_t* m_dev, const uint64_t theta[4], const uint64_t beta[4],
                     uint64_t* b_coeff_dev, uint64_t* f_coeff_dev, uint64_t* commitments, uint64_t* a_at_zero);
/* The static-lookup part of Evaluator::evaluate_h (plonk/evaluation.rs:533-548; called at plonk/prover.rs:606-624):
 * h <- h * y + (b (f l_active_row + beta) - 1) per lookup on the extended coset, starting from h_in_dev (the gate /
 * permutation / legacy-lookup terms folded so far; NULL = zero); b and f are taken in coefficient form and extended here
 * (:535-536).  divide_by_vanishing != 0 also applies EvaluationDomain::divide_by_vanishing_poly (poly/domain.rs:319-338,
 * what vanishing::Argument::construct does next, vanishing/prover.rs:84).  h_out_dev: ext elements (may alias h_in_dev). */
int cq_quotient_dev(cq_pk* pk, const uint64_t* b_coeff_dev, const uint64_t* f_coeff_dev, const uint64_t y[4], const uint64_t beta[4],
                    const uint64_t* h_in_dev, int divide_by_vanishing, uint64_t* h_out_dev);
/* permute_expression_pair of the legacy (halo2) lookup argument, plonk/lookup/prover.rs:400-502, without the blinding rows
 * it appends (:486-497, the caller's RNG): the first `usable` rows of the compressed input expression sorted by canonical
 * value, and the compressed table expression rearranged so that every first occurrence of an input value faces the same
 * table value and the remaining table values fill the repeated rows the way the reference does (ascending values into
 * descending rows).  All arrays: device, Montgomery-form field elements; the outputs hold `usable` elements and may not
 * alias the inputs.  2^k >= usable is the domain size (sizes the sort).  CQ_ERR_LOOKUP when an input value is missing from
 * the table (Error::ConstraintSystemFailure, :456-460). */
int cq_permute_expression_pair_dev(cq_ctx* ctx, uint32_t k, uint32_t usable, const uint64_t* input_dev, const uint64_t* table_dev,
                                   uint64_t* permuted_input_dev, uint64_t* permuted_table_dev);
/* ---- the other heavy stages of create_proof on their own: with the calls above, every stage of a general circuit's
 * proof can be swapped in one by one (INTEGRATION.md has the whole call sequence).  They run the code cq_create_proof*
 * runs for the same stage (prover_stages.hip), on the key's domain, window tables and scratch buffers.  Shapes: n = 2^k,
 * ext = 2^extended_k, bf = blinding_factors, S = permutation sets = ceil(permutation columns / (cs_degree - 2)),
 * PL = legacy lookups of `pk` in cs.lookups order; field elements in Montgomery form, 4 limbs.  A sharded key
 * (cq_pk_set_sharding world > 1) is CQ_ERR_ARG for all four, as for cq_pk_check_witness.
 *
 * permutation::Argument::commit (plonk/permutation/prover.rs:47-198), called at plonk/prover.rs:539-549: per set the
 * grand product z over the set's columns (:106-166) starting from the previous set's last_z (:173), its bf blinding rows
 * (:169-171) and its blind (:175, unused by KZG) drawn from the RNG in that order, set after set; commit_lagrange (:177),
 * coefficient form (:179).  The fixed columns are the key's.
 *   advice_dev:   num_advice DEVICE columns of n Lagrange values, blinding rows included
 *   instance_dev: num_instance device columns of n Lagrange values, zero beyond the instance (NULL without instance columns)
 *   rng, rng_state: as for cq_create_proof; S x (bf + 1) x 8 words are drawn, through cq_pk_set_rng_fill's hook when set
 *   z_coeff_dev:  S x n elements out, the z polynomials in coefficient form (written when the call returns)
 *   commitments:  HOST, S affine points (8 limbs each), in write order
 * CQ_ERR_ARG for a key without a permutation argument. */
int cq_permutation_commit_dev(cq_pk* pk, const uint64_t* const* advice_dev, const uint64_t* const* instance_dev, const uint64_t beta[4],
                              const uint64_t gamma[4], cq_rng_next_u64 rng, void* rng_state, uint64_t* z_coeff_dev,
                              uint64_t* commitments);
/* lookup::Permuted::commit_product (plonk/lookup/prover.rs:173-318), called at plonk/prover.rs:552-560, for every legacy
 * lookup of the key: z = the running product of (A + beta)(S + gamma) / ((A' + beta)(S' + gamma)) (:187-258), its bf
 * blinding rows (:259) and its blind (:302) drawn from the RNG, lookup after lookup; commit_lagrange (:303), coefficient
 * form (:304).
 *   input_dev, table_dev: PL device pointers each, the theta-compressed input / table expressions, n Lagrange values
 *   permuted_input_dev, permuted_table_dev: PL device pointers each, n values: cq_permute_expression_pair_dev's output
 *       with the bf + 1 blinding rows of lookup/prover.rs:477-479 appended by the caller
 *   z_coeff_dev: PL x n elements out;  commitments: HOST, PL affine points
 * A key without legacy lookups: CQ_OK, nothing drawn or written. */
int cq_lookup_commit_product_dev(cq_pk* pk, const uint64_t* const* input_dev, const uint64_t* const* table_dev,
                                 const uint64_t* const* permuted_input_dev, const uint64_t* const* permuted_table_dev,
                                 const uint64_t beta[4], const uint64_t gamma[4], cq_rng_next_u64 rng, void* rng_state,
                                 uint64_t* z_coeff_dev, uint64_t* commitments);
/* The part of Evaluator::evaluate_h before the static lookups (plonk/evaluation.rs:285-531; called at
 * plonk/prover.rs:606-624): advice and instance polynomials onto the extended coset (:317-335), the custom gates folded
 * with y (:348-365), the permutation terms (:367-459), the legacy-lookup terms (:461-531).  h_out_dev is what
 * cq_quotient_dev takes as h_in_dev; for a key with none of the three it is all zero, and cq_quotient_dev then gives
 * what it gives for h_in_dev = NULL.  Asynchronous on the context's stream, except for a circuit with user challenges:
 * their upload is waited for before the call returns.
 *   advice_coeff_dev:   num_advice device polynomials, n coefficients;  instance_coeff_dev: num_instance of them (or NULL)
 *   perm_z_coeff_dev:   S x n, as left by cq_permutation_commit_dev (NULL when S = 0)
 *   permuted_input_coeff_dev, permuted_table_coeff_dev: PL device pointers each, A' and S' in coefficient form
 *   lookup_z_coeff_dev: PL x n, as left by cq_lookup_commit_product_dev (all three NULL when PL = 0)
 *   challenges:         HOST, num_challenges x 4 limbs (NULL without user challenges)
 *   h_out_dev:          ext elements out */
int cq_evaluate_h_dev(cq_pk* pk, const uint64_t* const* advice_coeff_dev, const uint64_t* const* instance_coeff_dev,
                      const uint64_t* perm_z_coeff_dev, const uint64_t* const* permuted_input_coeff_dev,
                      const uint64_t* const* permuted_table_coeff_dev, const uint64_t* lookup_z_coeff_dev, const uint64_t* challenges,
                      const uint64_t beta[4], const uint64_t gamma[4], const uint64_t theta[4], const uint64_t y[4], uint64_t* h_out_dev);
/* The multi-open argument for arbitrary queries, with the key's opener (cq_pk_set_opener): ProverGWC::create_proof
 * (poly/kzg/multiopen/gwc/prover.rs:42-91) or ProverSHPLONK::create_proof (shplonk/prover.rs:120-286), called at
 * plonk/prover.rs:775-778.  A query names a polynomial in coefficient form on the device (1 <= len <= n coefficients) and
 * a point; the evaluations are computed here.  Queries of one polynomial carry the same pointer and length (that is how
 * SHPLONK's construct_intermediate_sets, shplonk.rs:56-133, tells commitments apart); points are compared by value.  At
 * most 8 points per polynomial and 64 distinct point sets with SHPLONK.
 * The transcript stays with the caller: squeeze_challenge yields the next challenge scalar, write_point takes a
 * commitment (affine, 8 limbs), both return 0 or fail the call with CQ_ERR_ARG.  Call order: GWC squeezes v (:49), then
 * writes one witness commitment per distinct point in first-seen order (:85-87); SHPLONK squeezes y (:136) and v (:196),
 * writes the quotient commitment (:204), squeezes u (:206), writes the opening commitment (:270). */
typedef struct { const uint64_t* poly_dev; size_t len; uint64_t point[4]; } cq_open_query;
typedef int (*cq_squeeze_challenge_fn)(void* user, uint64_t* out /* 4 limbs */);
typedef int (*cq_write_point_fn)(void* user, const uint64_t* affine /* 8 limbs */);
typedef struct { cq_squeeze_challenge_fn squeeze_challenge; cq_write_point_fn write_point; void* user; } cq_open_transcript;
int cq_multiopen_dev(cq_pk* pk, const cq_open_query* queries, size_t count, const cq_open_transcript* transcript);
/* S and PL of the key: what sizes the buffers of the stage calls above. */
uint32_t cq_pk_permutation_sets(const cq_pk* pk);
uint32_t cq_pk_legacy_lookups(const cq_pk* pk);
/* The verifying-key commitments the prover's key implies: commit_lagrange of every fixed column
 * (keygen.rs:247-250) and of every permutation polynomial (permutation/keygen.rs:115-149), as affine
 * points (num_fixed x 8 and num_perm_columns x 8 words). */
int cq_pk_vk_commitments(cq_pk* pk, uint64_t* fixed_commitments, uint64_t* permutation_commitments);

/* ---- sha/src/tables.rs: SHA-256 word -> limb witness fill ----------------------------------------- */
/* Decomposes `nwords` 32-bit words (device) into 12/10/10-bit limbs (LongLimbs, tables.rs:70-75,
 * 135-154) and writes, for limb t, its dense value to column 2*(t % pairs) and its bit-spread value
 * (bit i -> bit 2i) to column 2*(t % pairs)+1 at row t / pairs, Montgomery-encoded.  `cols_dev`:
 * 2*pairs device columns of `n` elements, zero-filled by the caller. */
int cq_sha_witness_fill_dev(cq_ctx* ctx, const uint32_t* words_dev, size_t nwords, uint32_t pairs, size_t n,
                            uint64_t* const* cols_dev);
/* sha/src/tables.rs generators, rows of four u64 written to device memory:
 * create_{rot0,rot1,maj,ch}_table::<L> (tables.rs:105-133; kind 0..3), 2^(first+2*second) rows (x,y,z,f);
 * create_decomposition_table::<L,K> (tables.rs:135-154), 2^k_bits rows (a,x,y,z). */
int cq_sha_synthesis_table_dev(cq_ctx* ctx, int kind, uint32_t first_limb_len, uint32_t second_limb_len, uint64_t* out_dev);
int cq_sha_decomposition_table_dev(cq_ctx* ctx, uint32_t first_limb_len, uint32_t second_limb_len, uint32_t k_bits,
                                   uint64_t* out_dev);
/* dense[i] = i, spread[i] = bit-spread(i) for i < size (device arrays of `size` elements). */
int cq_sha_spread_table_dev(cq_ctx* ctx, size_t size, uint64_t* dense_dev, uint64_t* spread_dev);

/* ---- SHA-256 compression circuit: layout and witness synthesis (no counterpart in the reference) --------------- */
/* The circuit (sha2_on_cq_halo2_amd/sha256_circuit.py, DESIGN.md "SHA-256 compression circuit") is laid out in regions
 * of CQ_SHA256_REGION_ROWS rows over CQ_SHA256_ADVICE_COLUMNS advice columns: CQ_SHA256_PAIRS (dense, spread) column
 * pairs -- columns 2j and 2j+1 -- and two plain columns behind them.  A block takes CQ_SHA256_BLOCK_REGIONS regions:
 * four that hold the incoming state (a_-1 .. a_-4, e_-1 .. e_-4) and one per round; CQ_SHA256_TAIL_REGIONS more after
 * the last block hold the digest.  Every cell of a region is a bit field of one 32-bit word of that region (the
 * `kind`, CQ_SHA256_SRC_*), described once in csrc/sha256_layout.hpp; the synthesis kernel and the constraint system
 * both read that table, the latter through cq_sha256_layout.  A cell is CQ_SHA256_CELL_WORDS words
 * (kind, form, column, row, offset, per_table_bits, len):
 *   form    CQ_SHA256_FORM_WORD: the field itself at (column, row); CQ_SHA256_FORM_SPREAD: its bit-spread form
 *           (bit i -> bit 2i, a 64-bit value); CQ_SHA256_FORM_PAIR: the field at (column, row) and its bit-spread form
 *           at (column + 1, row), both looked up
 *   offset, per_table_bits, len    the field is bits [offset + per_table_bits * table_bits, .. + len) of the word;
 *           len = 0 stands for "table_bits bits, or as many as the word has left" (a chunk of an even / odd word) */
#define CQ_SHA256_REGION_ROWS 8
#define CQ_SHA256_BLOCK_REGIONS 68
#define CQ_SHA256_TAIL_REGIONS 4
#define CQ_SHA256_PAIRS 8
#define CQ_SHA256_ADVICE_COLUMNS 18
#define CQ_SHA256_MIN_TABLE_BITS 11
#define CQ_SHA256_MAX_TABLE_BITS 16
#define CQ_SHA256_FORM_WORD 0
#define CQ_SHA256_FORM_PAIR 1
#define CQ_SHA256_FORM_SPREAD 2
#define CQ_SHA256_SRC_A 0      /* a_r, the first working variable after round r (r < 0: the incoming state) */
#define CQ_SHA256_SRC_E 1      /* e_r */
#define CQ_SHA256_SRC_W 2      /* the schedule word W_r */
#define CQ_SHA256_SRC_S0_EVEN 3   /* Sigma0(a_r): the even (xor) and odd (carry) bits of the three rotations' sum */
#define CQ_SHA256_SRC_S0_ODD 4
#define CQ_SHA256_SRC_S1_EVEN 5   /* Sigma1(e_r) */
#define CQ_SHA256_SRC_S1_ODD 6
#define CQ_SHA256_SRC_MAJ_EVEN 7  /* a_r + a_(r-1) + a_(r-2) bitwise: odd = Maj */
#define CQ_SHA256_SRC_MAJ_ODD 8
#define CQ_SHA256_SRC_CHP_EVEN 9  /* e_r + e_(r-1) bitwise: odd = e_r & e_(r-1) */
#define CQ_SHA256_SRC_CHP_ODD 10
#define CQ_SHA256_SRC_CHQ_EVEN 11 /* ~e_r + e_(r-2) bitwise: odd = ~e_r & e_(r-2) */
#define CQ_SHA256_SRC_CHQ_ODD 12
#define CQ_SHA256_SRC_G0_EVEN 13  /* sigma0(W_r) */
#define CQ_SHA256_SRC_G0_ODD 14
#define CQ_SHA256_SRC_G1_EVEN 15  /* sigma1(W_r) */
#define CQ_SHA256_SRC_G1_ODD 16
#define CQ_SHA256_SRC_CARRY_A 17  /* carry of the addition that gives a_r */
#define CQ_SHA256_SRC_CARRY_E 18  /* carry of the addition that gives e_r */
#define CQ_SHA256_SRC_CARRY_W 19  /* carry of the addition that gives W_r (rounds 16 .. 63) */
#define CQ_SHA256_SRC_K 20        /* the witness copy of the round constant K_r */
#define CQ_SHA256_SRC_CH 21       /* Ch(e_r, e_(r-1), e_(r-2)) = the two odd words above, added */
#define CQ_SHA256_SRC_COUNT 22
#define CQ_SHA256_CELL_WORDS 7 /* a cell of the layout table: kind, form, column, row, offset, per_table_bits, len */
/* Host only: writes the first `cap` cells of the layout table to `cells` (CQ_SHA256_CELL_WORDS words each; may be NULL
 * with cap = 0) and the number of cells the table has to *count. */
int cq_sha256_layout(uint32_t* cells, size_t cap, size_t* count);
/* Fills the CQ_SHA256_ADVICE_COLUMNS advice columns of the circuit for `blocks` chained 64-byte blocks on the context's
 * stream: `msg_words` are the 16 * blocks big-endian words of the padded message (host memory), `cols_dev` device columns
 * of `n` elements each; every row is written, Montgomery-encoded, the rows behind the
 * (CQ_SHA256_BLOCK_REGIONS * blocks + CQ_SHA256_TAIL_REGIONS) * CQ_SHA256_REGION_ROWS the layout uses with zero.  The
 * compression chain runs on the host (64 sequential rounds per block); a kernel expands its (a, e, W) words into the
 * cells.  `digest` receives the eight words of SHA-256's output, which the last four regions hold.  CQ_ERR_ARG:
 * table_bits outside [CQ_SHA256_MIN_TABLE_BITS, CQ_SHA256_MAX_TABLE_BITS], or n too small for the rows used. */
int cq_sha256_synthesize_dev(cq_ctx* ctx, uint32_t table_bits, const uint32_t* msg_words, size_t blocks, size_t n,
                             uint64_t* const* cols_dev, uint32_t digest[8]);
/* Several compression chains ("segments") one behind another in the same columns, wired to each other: segment j takes
 * CQ_SHA256_BLOCK_REGIONS * seg_blocks[j] + CQ_SHA256_TAIL_REGIONS regions directly behind segment j - 1, and its first
 * block starts from the IV.  `sources` holds one word per message word, 16 per block, in row order over all segments
 * (16 * sum(seg_blocks) words): a value below CQ_SHA256_SOURCE_DIGEST is an index into `words_dev`, a device array of
 * `words_len` 32-bit words (private words and constants alike); CQ_SHA256_SOURCE_DIGEST + 8 * s + i is digest word i of
 * segment s, which must come before the segment that reads it.  `digests_dev` (device, 8 * segments words) receives every
 * segment's digest.  All of it is validated on the host before anything is launched: CQ_ERR_ARG -- with the segment and
 * the word in cq_last_error -- for a block count of zero, rows that do not fit n, an index outside `words_dev`, a
 * reference to the segment itself or a later one, or table_bits out of range; nothing is written then.
 * The chains run on the device: a segment's level is 0 if it reads no digest, else one more than the highest level it
 * reads; one launch per level in ascending order, one lane per segment, then the expansion kernel of
 * cq_sha256_synthesize_dev over all rows (rows behind the last segment: zero).  Everything is queued on the context's
 * stream and nothing waits for it: `words_dev` must stay as it is, and `digests_dev` is good, once the stream has got
 * there.  A one-segment description gives the columns cq_sha256_synthesize_dev gives for the same words. */
#define CQ_SHA256_SOURCE_DIGEST 2147483648u
int cq_sha256_synthesize_segments_dev(cq_ctx* ctx, uint32_t table_bits, const uint32_t* seg_blocks, size_t segments,
                                      const uint32_t* sources, const uint32_t* words_dev, size_t words_len, size_t n,
                                      uint64_t* const* cols_dev, uint32_t* digests_dev);
/* The same with message words that are a choice between two operands under a private bit (DESIGN.md "Choice-wired message
 * words").  A source value CQ_SHA256_SOURCE_CHOICE + c (the digest flag is tested first) means entry c of `choices`, a host
 * array of `n_choices` entries of four words {bit, zero, one, 0}: `bit` is an index into `words_dev` of a word that is 0 or
 * 1; `zero` and `one` are plain sources -- a word index or a digest reference -- and the message word is `one` if the bit
 * word is not zero, else `zero`.  Every entry must be referenced by exactly one message word, whose region it then belongs
 * to: after the expansion a kernel writes the zero operand, the one operand and the bit word as given (a bit word that is
 * neither 0 nor 1 is the witness checker's finding, not an error here) to rows CQ_SHA256_CHOICE_ROW_ZERO / _ONE / _BIT of
 * that region in advice column CQ_SHA256_ADVICE_COLUMNS - 1, which the expansion leaves zero.  A segment's level also
 * counts the digests its choices read.  With n_choices > 0, words_len must not exceed CQ_SHA256_SOURCE_CHOICE.
 * CQ_ERR_ARG, besides the cases above and again before anything is queued: a choice index >= n_choices, an entry
 * referenced twice or never, a bit or operand index outside `words_dev`, a digest operand of the segment itself or a
 * later one.  n_choices = 0 (`choices` may be NULL) is cq_sha256_synthesize_segments_dev exactly. */
#define CQ_SHA256_SOURCE_CHOICE 1073741824u
#define CQ_SHA256_CHOICE_WORDS 4
#define CQ_SHA256_CHOICE_ROW_ZERO 4
#define CQ_SHA256_CHOICE_ROW_ONE 5
#define CQ_SHA256_CHOICE_ROW_BIT 6
int cq_sha256_synthesize_choices_dev(cq_ctx* ctx, uint32_t table_bits, const uint32_t* seg_blocks, size_t segments,
                                     const uint32_t* sources, const uint32_t* choices, size_t n_choices, const uint32_t* words_dev,
                                     size_t words_len, size_t n, uint64_t* const* cols_dev, uint32_t* digests_dev);
/* The same with segments that start from a wired state instead of the IV (DESIGN.md "Wired initial states").
 * `init_sources` is a host array of 8 entries per segment, H[0..7] of the state the segment's first block starts from: an
 * entry is CQ_SHA256_SOURCE_IV (tested before the digest flag) for the IV's word of that position, or a plain source -- a
 * word index or a digest reference.  A segment's level also counts the digests its initial words read: a segment whose
 * only dependency is its initial state still runs one level behind its producer.  CQ_ERR_ARG, besides the cases above and
 * again before anything is queued, with "segment j, initial word i" in cq_last_error: a digest of the segment itself or a
 * later one, an index outside `words_dev`, and -- with n_choices > 0 -- a value at or above CQ_SHA256_SOURCE_CHOICE (a
 * choice is no initial word).  init_sources = NULL is cq_sha256_synthesize_choices_dev exactly. */
#define CQ_SHA256_SOURCE_IV 4294967295u
int cq_sha256_synthesize_states_dev(cq_ctx* ctx, uint32_t table_bits, const uint32_t* seg_blocks, size_t segments,
                                    const uint32_t* sources, const uint32_t* choices, size_t n_choices, const uint32_t* init_sources,
                                    const uint32_t* words_dev, size_t words_len, size_t n, uint64_t* const* cols_dev,
                                    uint32_t* digests_dev);
/* The same with message words that are the XOR of two plain sources (DESIGN.md "XOR-wired message words").  `xors` is a
 * host array of `n_xors` units of CQ_SHA256_XOR_WORDS words {x, y, 0, 0}: x and y are plain sources -- a word index or a
 * digest reference to a segment that exists; no unit's result and no choice.  `digests_dev` holds 8 * segments + n_xors
 * words: word 8 * segments + u receives x ^ y of unit u, and a message word reads it through the source value
 * CQ_SHA256_SOURCE_DIGEST + 8 * segments + u (a message word's own source only: not an operand of a choice, not an initial
 * word).  Any number of message words may read one unit, none included.  Unit u takes CQ_SHA256_XOR_REGIONS regions
 * directly behind the last segment's tail, regions R + 2u and R + 2u + 1 (R: the segments' regions): the first holds
 * e = x and nothing else, the second e = y and W = x ^ y, with the Ch cells of two consecutive e words that the expansion
 * lays out for it.  A unit is ready at level 0 if it reads no digest, else one level above the highest level it reads; a
 * segment that reads a unit runs at or above the unit's level.  Per level one launch computes that level's units before
 * the level's chains, and one more behind the last level those over its digests; then the expansion runs once over all
 * regions.  CQ_ERR_ARG, besides the cases above and again before anything is queued, naming the unit (and segment and
 * word for a reader): an operand index outside `words_dev`, a digest operand of a segment that does not exist, a reader
 * in segment j of a unit with a digest operand of segment >= j, a unit index >= n_xors, an area that does not fit n.
 * n_xors = 0 (`xors` may be NULL) is cq_sha256_synthesize_states_dev exactly. */
#define CQ_SHA256_XOR_WORDS 4
#define CQ_SHA256_XOR_REGIONS 2
int cq_sha256_synthesize_xors_dev(cq_ctx* ctx, uint32_t table_bits, const uint32_t* seg_blocks, size_t segments,
                                  const uint32_t* sources, const uint32_t* choices, size_t n_choices, const uint32_t* init_sources,
                                  const uint32_t* xors, size_t n_xors, const uint32_t* words_dev, size_t words_len, size_t n,
                                  uint64_t* const* cols_dev, uint32_t* digests_dev);
/* Messages of variable length with constrained padding (DESIGN.md "Variable-length messages"): segment j is a chain of
 * seg_max_blocks[j] blocks that holds message j -- msg_lens[j] raw bytes at msg_bytes_dev + msg_offsets[j], a device buffer
 * of msg_bytes_len bytes (no alignment is asked of it) -- padded on the device: 0x80, zeros, the bit length in the last two
 * words of the first block that has room for them (the FINAL block), zero words behind it.  Behind the chains and the
 * expansion of cq_sha256_synthesize_segments_dev a kernel writes the cells the padding gates read, which the expansion
 * leaves zero: in a message-word region (rounds 0 .. 15) rows CQ_SHA256_VAR_ROW_M / _LEN / _C0 / _C1 of the last advice
 * column (the word lies wholly inside the message; the running byte length; the two bits of 3 - (bytes of the message
 * in the boundary word)), the bits' product in the dense and spread cells of pair slot CQ_SHA256_VAR_SLOT_PRODUCT, row 0,
 * and the two 12-bit halves of the boundary word's message bytes in pair slot CQ_SHA256_VAR_SLOT_DATA, rows 0 and 1; in
 * region CQ_SHA256_VAR_REGION_CARRY of a block the flag and the length the block starts from (rows _M, _LEN) and their
 * factors; in regions CQ_SHA256_VAR_REGION_SUM + i (i < 8: digest word i) and CQ_SHA256_VAR_REGION_LENGTH rows
 * CQ_SHA256_VAR_ROW_IN / _FLAG / _VALUE / _OUT (out = in + flag * value: the word selected so far, whether the block is
 * the final one, the chaining value behind the block or the length); in region CQ_SHA256_VAR_REGION_FINAL rows _IN, _FLAG,
 * _VALUE hold the flags of word 13 of the block before and of this block and their difference.  `digests_dev` (8 * segments
 * words) receives the chaining value behind each message's final block: SHA-256 of the message.  Everything is validated
 * on the host before anything is queued; CQ_ERR_ARG, with the segment in cq_last_error: table_bits below
 * CQ_SHA256_VAR_MIN_TABLE_BITS or above CQ_SHA256_MAX_TABLE_BITS, a block count of zero, msg_lens[j] above
 * 64 * seg_max_blocks[j] - 9, an offset or a length that leaves the buffer, rows that do not fit n.  Nothing waits for the
 * stream: the buffer must stay as it is, and `digests_dev` is good, once the stream has got there. */
#define CQ_SHA256_VAR_MIN_TABLE_BITS 12
#define CQ_SHA256_VAR_ROW_M 4
#define CQ_SHA256_VAR_ROW_LEN 5
#define CQ_SHA256_VAR_ROW_C0 6
#define CQ_SHA256_VAR_ROW_C1 7
#define CQ_SHA256_VAR_SLOT_PRODUCT 6
#define CQ_SHA256_VAR_SLOT_DATA 7
#define CQ_SHA256_VAR_ROW_IN 4
#define CQ_SHA256_VAR_ROW_FLAG 5
#define CQ_SHA256_VAR_ROW_VALUE 6
#define CQ_SHA256_VAR_ROW_OUT 7
#define CQ_SHA256_VAR_REGION_CARRY 3
#define CQ_SHA256_VAR_REGION_SUM 20
#define CQ_SHA256_VAR_REGION_FINAL 28
#define CQ_SHA256_VAR_REGION_LENGTH 29
int cq_sha256_synthesize_varlen_dev(cq_ctx* ctx, uint32_t table_bits, const uint32_t* seg_max_blocks, size_t segments,
                                    const uint8_t* msg_bytes_dev, size_t msg_bytes_len, const uint64_t* msg_offsets,
                                    const uint64_t* msg_lens, size_t n, uint64_t* const* cols_dev, uint32_t* digests_dev);
/* The same continued from a state: segment j starts from the eight words at init_states_dev + 8 j (device, 8 * segments
 * words) instead of the IV, after base_lens[j] bytes (host) that the state has absorbed already.  The padding's length word
 * is the bit length of base_lens[j] + msg_lens[j]; every running-length cell, the carry-in of the first block and the
 * selected length count from the base.  CQ_ERR_ARG, besides the cases above, with the segment in cq_last_error: a base that
 * is no multiple of 64, or base_lens[j] + 64 * seg_max_blocks[j] above 2^29 (the bit length is the 32-bit word 15 of the
 * final block; word 14 is zero).  All-IV states with bases of zero give cq_sha256_synthesize_varlen_dev's columns. */
int cq_sha256_synthesize_varlen_from_dev(cq_ctx* ctx, uint32_t table_bits, const uint32_t* seg_max_blocks, size_t segments,
                                         const uint8_t* msg_bytes_dev, size_t msg_bytes_len, const uint64_t* msg_offsets,
                                         const uint64_t* msg_lens, const uint32_t* init_states_dev, const uint64_t* base_lens, size_t n,
                                         uint64_t* const* cols_dev, uint32_t* digests_dev);

/* ---- SHA-512 / SHA-384 compression circuit: layout and witness synthesis (no counterpart in the reference) ------ */
/* The 64-bit counterpart (sha2_on_cq_halo2_amd/sha512_circuit.py, DESIGN.md "SHA-512 and SHA-384 circuits"): the same
 * CQ_SHA256_ADVICE_COLUMNS advice columns -- CQ_SHA256_PAIRS (dense, spread) pairs and two plain columns -- in regions
 * of CQ_SHA512_REGION_ROWS rows.  A block of 128 bytes takes CQ_SHA512_BLOCK_REGIONS regions: four that hold the
 * incoming state and one per round (80); CQ_SHA512_TAIL_REGIONS more after a message's last block hold its final state.
 * Every cell is a bit field of one 64-bit word of its region, by the table of csrc/sha512_layout.hpp: the cell record,
 * the CQ_SHA256_SRC_* word kinds and the CQ_SHA256_FORM_* forms are those of cq_sha256_layout, with these differences:
 * a word has 64 bits, so a CQ_SHA256_FORM_SPREAD cell is a 128-bit value; an even / odd word has CQ_SHA512_CHUNKS chunks
 * of table_bits bits, of which those that start at or above bit 64 hold zero (6, 5, 4 non-empty chunks at table_bits
 * 11 .. 12, 13 .. 15 and 16); CQ_SHA256_SRC_CARRY_W is the carry of rounds 16 .. 79. */
#define CQ_SHA512_REGION_ROWS 16
#define CQ_SHA512_BLOCK_REGIONS 84
#define CQ_SHA512_TAIL_REGIONS 4
#define CQ_SHA512_MIN_TABLE_BITS 11
#define CQ_SHA512_MAX_TABLE_BITS 16
#define CQ_SHA512_CHUNKS 6
#define CQ_SHA512_VARIANT_512 0 /* a segment starts from SHA-512's initial hash value */
#define CQ_SHA512_VARIANT_384 1 /* ... from SHA-384's; the digest is the first six words of the final state */
/* Host only: writes the first `cap` cells of the layout table to `cells` (CQ_SHA256_CELL_WORDS words each; may be NULL
 * with cap = 0) and the number of cells the table has to *count. */
int cq_sha512_layout(uint32_t* cells, size_t cap, size_t* count);
/* Fills the CQ_SHA256_ADVICE_COLUMNS advice columns for `segments` independent messages one behind another: segment j
 * takes CQ_SHA512_BLOCK_REGIONS * seg_blocks[j] + CQ_SHA512_TAIL_REGIONS regions directly behind segment j - 1 and starts
 * from the initial hash value seg_variant[j] names (CQ_SHA512_VARIANT_*).  `msg_words` (host) are the big-endian 64-bit
 * words of the padded messages back to back, 16 per block; `cols_dev` device columns of `n` elements each: every row
 * below n is written, Montgomery-encoded, the rows behind the last segment's regions with zero; no row at or behind n is
 * touched.  The compression chains run on the device, one lane per segment, and leave (a, e, W, kind) per region there
 * for the expansion kernel, one thread per row; both are queued on the context's stream behind the words' upload, and the
 * call waits for the stream once, at its end.  `digests_out` (host, 8 * segments words) receives every segment's final
 * state, eight words whatever the variant.  All arguments are checked on the host before anything is launched:
 * CQ_ERR_ARG -- with the segment in cq_last_error -- for table_bits outside [CQ_SHA512_MIN_TABLE_BITS,
 * CQ_SHA512_MAX_TABLE_BITS], no segment, a block count of zero, a variant that is neither of the two, or n too small
 * for the rows used; nothing is written then. */
int cq_sha512_synthesize_dev(cq_ctx* ctx, uint32_t table_bits, const uint32_t* seg_blocks, size_t segments,
                             const uint32_t* seg_variant, const uint64_t* msg_words, size_t n, uint64_t* const* cols_dev,
                             uint64_t* digests_out);
/* The same for segments wired to each other (sha2_on_cq_halo2_amd/sha512_segments.py, DESIGN.md "Wired SHA-512
 * segments"): the 64-bit counterpart of cq_sha256_synthesize_states_dev without choices.  `sources` (host) holds one
 * entry per message word, 16 per block, in row order over all segments: a value below CQ_SHA512_SOURCE_DIGEST is an index
 * into `words_dev`, a device array of `words_len` 64-bit words (private words and constants alike);
 * CQ_SHA512_SOURCE_DIGEST + 8 * s + i is word i of the final state of segment s, which must come before the segment that
 * reads it -- all eight words are readable whatever the variant of s.  `init_sources` (host, 8 entries per segment, or NULL
 * for the initial hash value everywhere) is H[0..7] of the state a segment's first block starts from: CQ_SHA512_SOURCE_IV
 * (tested before the digest flag) for the word of seg_variant[j]'s initial hash value at that position, or a source as
 * above.  `digests_dev` (device, 8 * segments words) receives every segment's final state.  A segment that reads no
 * digest is of level 0, any other one level above the highest it reads -- through a message word or an initial word
 * alike; the chains run one launch per level in ascending order, one lane per segment, then the expansion over all rows.
 * Everything is queued on the context's stream and nothing waits for it: `words_dev` must stay as it is, and
 * `digests_dev` is good, once the stream has got there.  All of it is validated on the host before anything is queued:
 * CQ_ERR_ARG -- with "segment j, word t" or "segment j, initial word i" in cq_last_error where one is at fault -- for a
 * null array, no segment, a block count of zero, a variant that is neither of the two, table_bits out of range, regions
 * that do not fit n, a word index at or above words_len, a digest of the segment itself or a later one, and
 * CQ_SHA512_SOURCE_IV among `sources`; nothing is written then.  A description whose words are all private and whose
 * init_sources is NULL gives the columns and digests cq_sha512_synthesize_dev gives for the same words. */
#define CQ_SHA512_SOURCE_DIGEST 2147483648u
#define CQ_SHA512_SOURCE_IV 4294967295u
int cq_sha512_synthesize_segments_dev(cq_ctx* ctx, uint32_t table_bits, const uint32_t* seg_blocks, size_t segments,
                                      const uint32_t* seg_variant, const uint32_t* sources, const uint32_t* init_sources,
                                      const uint64_t* words_dev, size_t words_len, size_t n, uint64_t* const* cols_dev,
                                      uint64_t* digests_dev);
/* The same with message words that are the XOR of two plain sources (sha2_on_cq_halo2_amd/sha512_xor.py, DESIGN.md
 * "XOR-wired message words on the 64-bit circuit"): the 64-bit counterpart of cq_sha256_synthesize_xors_dev.  `xors` is a
 * host array of `n_xors` units of CQ_SHA512_XOR_WORDS words {x, y, 0, 0}: x and y are plain sources -- a word index or a
 * digest reference to a segment that exists; no unit's result.  `digests_dev` holds 8 * segments + n_xors 64-bit words:
 * word 8 * segments + u receives x ^ y of unit u, and a message word reads it through the source value
 * CQ_SHA512_SOURCE_DIGEST + 8 * segments + u (a message word's own source only: not an initial word).  Any number of
 * message words may read one unit, none included.  Unit u takes CQ_SHA512_XOR_REGIONS regions directly behind the last
 * segment's tail, regions R + 2u and R + 2u + 1 (R: the segments' regions): the first holds e = x and nothing else, the
 * second e = y and W = x ^ y, with the Ch cells of two consecutive e words that the expansion lays out for it.  A unit is
 * ready at level 0 if it reads no digest, else one level above the highest level it reads; a segment that reads a unit
 * runs at or above the unit's level.  Per level one launch computes that level's units before the level's chains, and one
 * more behind the last level those over its digests; then the expansion runs once over all regions.  CQ_ERR_ARG, besides
 * the cases above and again before anything is queued, naming the unit (and segment and word for a reader): a null table
 * with n_xors > 0, an operand index outside `words_dev`, a digest operand of a segment that does not exist, a reader in
 * segment j of a unit with a digest operand of segment >= j, a unit index >= n_xors, an area that does not fit n.
 * n_xors = 0 (`xors` may be NULL) is cq_sha512_synthesize_segments_dev exactly. */
#define CQ_SHA512_XOR_WORDS 4
#define CQ_SHA512_XOR_REGIONS 2
int cq_sha512_synthesize_xors_dev(cq_ctx* ctx, uint32_t table_bits, const uint32_t* seg_blocks, size_t segments,
                                  const uint32_t* seg_variant, const uint32_t* sources, const uint32_t* init_sources,
                                  const uint32_t* xors, size_t n_xors, const uint64_t* words_dev, size_t words_len, size_t n,
                                  uint64_t* const* cols_dev, uint64_t* digests_dev);

/* ---- harness RNG (not in the reference: its test draws from OsRng) ---------------------------------- */
void cq_xoshiro256ss_seed(uint64_t seed, uint64_t state[4]);
uint64_t cq_xoshiro256ss_next_u64(void* state /* uint64_t[4] */);
/* `count` consecutive outputs of the generator above into dst, advancing the state -- the same words and final state
 * as `count` calls of cq_xoshiro256ss_next_u64, produced by up to `threads` host threads (jump-ahead on the
 * GF(2)-linear state transition).  cq_create_proof* draws the vanishing argument's random polynomial this way
 * (8 * 2^k words: the RNG, not the GPU, bounds the first rounds of a large proof otherwise). */
void cq_xoshiro256ss_fill(uint64_t state[4], uint64_t* dst, size_t count, uint32_t threads);
/* replays a pre-drawn stream: state = {const uint64_t* words; size_t pos; size_t len; size_t overrun}.  Words asked
 * for beyond `len` read as zero and are counted in `overrun` (reset by cq_create_proof* when a proof starts: the
 * caller need not initialise it); cq_create_proof* fails with CQ_ERR_ARG when the stream it was given ran out (a proof
 * blinded with zeros is not zero-knowledge); an unrelated failure (e.g. CQ_ERR_LOOKUP) keeps its own code.  Like the xoshiro generator below this is
 * for tests and benches; production blinding comes from the caller's CSPRNG through cq_rng_next_u64. */
typedef struct { const uint64_t* words; size_t pos; size_t len; size_t overrun; } cq_buffer_rng;
uint64_t cq_buffer_rng_next_u64(void* state /* cq_buffer_rng* */);
/* The xoshiro generator behind a function the library does NOT recognise (state: uint64_t[4]): stands in for a
 * caller's opaque `RngCore` in tests and in bench.py's `generic_rng` leg (same words as cq_xoshiro256ss_next_u64). */
uint64_t cq_opaque_rng_next_u64(void* state);
void cq_opaque_rng_fill(void* state, uint64_t* dst, size_t count);

/* ---- measurement support ---------------------------------------------------------------------- */
/* When enabled, the library brackets its dominant kernels with HIP events on the context's stream.
 * cq_profile_read drains the stream and returns the summed duration and launch count for `id`
 * (and forgets those spans). */
#define CQ_PROF_MSM_ACCUMULATE 1 /* msm_accumulate_kernel: bucket accumulation (mixed additions) */
#define CQ_PROF_NTT_PASS 2       /* ntt_pass_kernel: one radix-2^deg Stockham pass */
#define CQ_PROF_MSM_ENTRIES 3    /* no timing: `calls` = (point, non-zero digit) pairs = mixed additions executed by
                                  * msm_accumulate_kernel since the last read */
#define CQ_PROF_G1_DECOMPRESS 4  /* g1_decompress_kernel: point decompression of the Processed readers */
#define CQ_PROF_G2_DECOMPRESS 5  /* g2_decompress_kernel: G2 point decompression (params tail, G2 SRS) */
int cq_profile_enable(cq_ctx* ctx, int on);
int cq_profile_read(cq_ctx* ctx, int id, double* total_ms, uint64_t* calls);

/* ---- microbenchmarks (measurement support, not part of the drop-in surface) -------------- */
/* Runs `iters` dependent Montgomery multiplications per lane over `lanes` lanes and writes one
 * folded element per lane; used to measure the chip's 256-bit modmul rate. which: 0 = Fr, 1 = Fq (the 8 x u32
 * memory-format type), 2 = Fq in the lazy 9 x 29-bit form the MSM kernels compute in */
int cq_bench_modmul_dev(cq_ctx* ctx, uint64_t* out_dev, uint32_t lanes, uint32_t iters, int which);

#ifdef __cplusplus
}
#endif
#endif /* CQ_HALO2_H */

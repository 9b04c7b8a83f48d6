"""`ProvingKey`: keygen's output on the GPU, `create_proof` in its forms, the prover's stages on their own, the witness
checker (`MockProver`) and sharding across ranks."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from ._lib import CqError
from ._marshal import (FAIL_GATE, FAIL_GATE_POISONED, FAIL_LOOKUP, FAIL_PERMUTATION, FAIL_STATIC_LOOKUP, SERDE_PROCESSED,
                       _ALLGATHER_T, _BCAST_T, _EXCHANGE_T, _OPENERS, _PHASE_T, _SQUEEZE_T, _WRITE_POINT_T, _BufferRng, _CqCircuit,
                       _CqOpenQuery, _CqOpenTranscript, _CqPlonk, _ProofBuffer, _assigned_structs, _fr, _g1, _instance_columns,
                       _limbs4, _ptr_array, _struct_of, _written, fr_from_mont, fr_to_mont)
from .context import Context, DevBuf, _Handle
from .params import ParamsKZG, TableConfig


def _lower_plonk(cs, fixed, mapping, keep: list, from_raw: bool = False) -> _CqPlonk:
    """`ConstraintSystem` (+ the keygen outputs `fixed_values`, `Assembly.mapping`) -> cq_plonk arrays.
    from_raw: the key's polynomials come from a serialized ProvingKey, only the shape is lowered."""
    pl = _CqPlonk()
    n_fixed = cs.num_fixed_columns
    fixed = [_fr(f) for f in (fixed or [])]
    pl.num_fixed, pl.num_instance = n_fixed, cs.num_instance_columns
    if not from_raw:
        assert len(fixed) == n_fixed, "one value column per fixed column (pk.fixed_values)"
        fptrs = _ptr_array([f.ctypes.data for f in fixed], False)
        keep += [fixed, fptrs]
        pl.fixed = C.cast(fptrs, C.POINTER(C.c_void_p))
    pl.cs_degree, pl.blinding_factors = cs.degree(), cs.blinding_factors()

    def words(ty, vals):
        a = (ty * max(len(vals), 1))(*vals)
        keep.append(a)
        return C.cast(a, C.POINTER(ty))

    def u32(vals):
        return words(C.c_uint32, vals)

    pl.num_advice_queries = len(cs.advice_queries)
    pl.advice_query_columns = u32([c for c, _ in cs.advice_queries])
    pl.advice_query_rotations = words(C.c_int32, [r for _, r in cs.advice_queries])
    pl.num_fixed_queries = len(cs.fixed_queries)
    pl.fixed_query_columns = u32([c for c, _ in cs.fixed_queries])
    pl.fixed_query_rotations = words(C.c_int32, [r for _, r in cs.fixed_queries])
    constants = []

    def programs(exprs):
        """(words per program, the programs back to back) of the expressions, as u32 arrays"""
        progs = [e.compile(constants) for e in exprs]
        return u32([len(p) for p in progs]), u32([w for p in progs for w in p])

    pl.num_gate_polys = len(cs.gates)
    pl.gate_program_lens, pl.gate_programs = programs(cs.gates)
    if cs.static_lookup_inputs is not None:  # expression-valued lookup inputs
        pl.lookup_input_program_lens, pl.lookup_input_programs = programs(cs.static_lookup_inputs)
    if cs.lookups:  # legacy lookups: per lookup the input programs, then the table programs
        pl.num_legacy_lookups, pl.legacy_lookup_widths = len(cs.lookups), u32([len(ins) for ins, _ in cs.lookups])
        pl.legacy_program_lens, pl.legacy_programs = programs([e for ins, tabs in cs.lookups for e in list(ins) + list(tabs)])
    if any(cs.advice_column_phase) or cs.challenge_phase:
        pl.advice_column_phases = words(C.c_uint8, cs.advice_column_phase)
        pl.num_challenges, pl.challenge_phases = len(cs.challenge_phase), words(C.c_uint8, cs.challenge_phase)
    cst = np.zeros((max(len(constants), 1), 4), dtype=np.uint64)
    for i, v in enumerate(constants):
        cst[i] = fr_to_mont(v)
    keep.append(cst)
    pl.num_constants, pl.constants = len(constants), cst.ctypes.data_as(C.POINTER(C.c_uint64))
    pl.num_perm_columns = len(cs.permutation_columns)
    pl.perm_column_kinds = u32([c.kind for c in cs.permutation_columns])
    pl.perm_column_indices = u32([c.index for c in cs.permutation_columns])
    if mapping is not None and len(cs.permutation_columns):  # (an Assembly over no columns has an empty mapping)
        m = np.ascontiguousarray(mapping, dtype=np.uint32)
        if m.ndim != 3 or m.shape[0] != len(cs.permutation_columns) or m.shape[2] != 2:
            raise CqError(-1, "permutation mapping: expected [columns][rows][2]")
        keep.append(m)
        pl.perm_mapping = m.ctypes.data_as(C.POINTER(C.c_uint32))
    return pl


class WitnessFailure(NamedTuple):
    """One finding of `ProvingKey.check_witness`: cq_witness_failure (kind = CQ_FAIL_*)."""

    kind: int
    index: int
    row: int
    detail: int = 0

    def __str__(self):
        if self.kind == FAIL_GATE:
            return f"gate polynomial {self.index} is not satisfied on row {self.row}"
        if self.kind == FAIL_GATE_POISONED:
            return f"gate polynomial {self.index} is poisoned on row {self.row} (it reads a blinding-row advice cell)"
        if self.kind == FAIL_LOOKUP:
            return f"lookup {self.index}: the inputs of row {self.row} are not a row of the table"
        if self.kind == FAIL_STATIC_LOOKUP:
            why = ("the value is not in the table", "the values are on different table rows", "the input is poisoned")[min(self.detail, 2)]
            return f"static lookup {self.index}, row {self.row}: {why}"
        if self.kind == FAIL_PERMUTATION:
            return f"permutation column {self.index}, row {self.row}: the cell differs from the one it is copied from"
        return f"finding of kind {self.kind} (index {self.index}, row {self.row})"


class WitnessError(CqError):
    """The witness does not satisfy the circuit: `total` findings, the first of them in `failures`."""

    def __init__(self, total, failures):
        more = f" (and {total - len(failures)} more)" if total > len(failures) else ""
        super().__init__(0, f"witness not satisfied, {total} finding(s): " + "; ".join(str(f) for f in failures) + more)
        self.total, self.failures = total, failures


class ProvingKey(_Handle):
    """The slice of `ProvingKey` (plonk.rs:291-308) that `create_proof` reads.

    lookups: list of lookups, each a list of (advice column, StaticTable).  For a general circuit pass
    `cs` (a `plonk.ConstraintSystem`: gates, fixed / instance columns, permutation columns; its static
    lookups and advice column count replace `lookups` / `num_advice`), `fixed` (pk.fixed_values) and
    `permutation` (`Assembly.mapping`); table_cfg / b0_g1_bound may be None without static lookups."""

    _destroy = "cq_pk_destroy"
    _close_first = True

    # ---- plonk.rs, plonk/keygen.rs: keygen_pk, ProvingKey::read / write ----
    def __init__(self, ctx: Context, params: ParamsKZG, k: int, num_advice: int, lookups, table_cfg: TableConfig,
                 b0_g1_bound, vk_repr: np.ndarray, cs=None, fixed=None, permutation=None, raw: bytes = None,
                 num_selectors: int = 0, checked: bool = None, format: int = None):
        self.params, self.k = params, k
        self.cs = cs
        if cs is not None:
            num_advice, lookups = cs.num_advice_columns, cs.static_lookups
        self._keep = [params, table_cfg, [t for lk in lookups for _, t in lk]]
        widths = (C.c_uint32 * max(len(lookups), 1))(*[len(lk) for lk in lookups])
        flat_cols = [c for lk in lookups for c, _ in lk]
        cols = (C.c_uint32 * max(len(flat_cols), 1))(*flat_cols)
        tabs = _ptr_array([t.h.value if isinstance(t.h, C.c_void_p) else t.h for lk in lookups for _, t in lk], False)
        cs_ = _CqCircuit()
        cs_.k, cs_.num_advice, cs_.num_lookups = k, num_advice, len(lookups)
        cs_.lookup_widths = C.cast(widths, C.POINTER(C.c_uint32))
        cs_.lookup_columns = C.cast(cols, C.POINTER(C.c_uint32))
        cs_.lookup_tables = C.cast(tabs, C.POINTER(C.c_void_p))
        cs_.vk_repr = tuple(int(v) for v in _limbs4(vk_repr))
        if cs is not None:
            pl = _lower_plonk(cs, fixed, permutation, self._keep, from_raw=raw is not None)
            self._keep.append(pl)
            cs_.plonk = C.pointer(pl)
        if b0_g1_bound is None:
            b0_ptr, on_dev = None, 0
        elif isinstance(b0_g1_bound, (int,)):
            b0_ptr, on_dev = b0_g1_bound, 1
        else:
            b0 = _g1(b0_g1_bound)
            assert b0.shape[0] == (1 << k) - 1, "b0_g1_bound must hold n-1 points (arithmetic.rs:133)"
            self._b0 = b0
            b0_ptr, on_dev = b0.ctypes.data, 0
        shape = (ctx.h, params.h, C.byref(cs_), table_cfg.h if table_cfg is not None else None, b0_ptr, on_dev)
        if raw is None:
            self._open(ctx, ctx.lib.cq_pk_create, *shape)
        else:
            rb = np.frombuffer(raw, dtype=np.uint8)
            if format is not None:  # `ProvingKey::read(reader, format)` in any SerdeFormat (ProvingKey.read)
                if checked is not None:
                    raise CqError(-1, "ProvingKey: give `format` or `checked`, not both")
                self._open(ctx, ctx.lib.cq_pk_read, *shape, rb.ctypes.data, rb.shape[0], num_selectors, format)
            else:  # `ProvingKey::read(reader, RawBytes | RawBytesUnchecked)` (plonk.rs:379-403); checked: default True
                checked = True if checked is None else checked
                self._open(ctx, ctx.lib.cq_pk_read_raw, *shape, rb.ctypes.data, rb.shape[0], num_selectors, 1 if checked else 0)
        self.num_advice = num_advice
        self._num_lookups = len(lookups)
        self._table_size = table_cfg.size if table_cfg is not None else 0
        self.usable_rows = ctx.lib.cq_pk_usable_rows(self.h)
        self.proof_size = ctx.lib.cq_pk_proof_size(self.h)

    @classmethod
    def read(cls, ctx: Context, params: ParamsKZG, k: int, num_advice: int, lookups, table_cfg, b0_g1_bound, vk_repr, data: bytes,
             format: int = SERDE_PROCESSED, cs=None, num_selectors: int = 0) -> "ProvingKey":
        """`ProvingKey::read(reader, format)` (plonk.rs:379-403): the constructor's arguments (the circuit's shape) plus the
        serialized key and its format."""
        return cls(ctx, params, k, num_advice, lookups, table_cfg, b0_g1_bound, vk_repr, cs=cs, raw=data, num_selectors=num_selectors,
                   format=format)

    def _write(self, size: int, fn, *fmt, selector_bits: bytes, num_selectors: int) -> bytes:
        sel = np.frombuffer(selector_bits, dtype=np.uint8) if num_selectors else None
        return _written(size, lambda buf, size, w: self.ctx._chk(fn(self.h, *fmt, sel.ctypes.data if sel is not None else None,
                                                                    num_selectors, buf, size, w)))

    def write(self, format: int = SERDE_PROCESSED, selector_bits: bytes = b"", num_selectors: int = 0) -> bytes:
        """`ProvingKey::write(writer, format)` (plonk.rs:349-362)."""
        return self._write(self.serialized_size(format, num_selectors), self.ctx.lib.cq_pk_write, format, selector_bits=selector_bits,
                           num_selectors=num_selectors)

    def to_bytes(self, selector_bits: bytes = b"", num_selectors: int = 0) -> bytes:
        """`ProvingKey::to_bytes(SerdeFormat::RawBytes)` (plonk.rs:405-410)."""
        return self._write(self.ctx.lib.cq_pk_raw_size(self.h, num_selectors), self.ctx.lib.cq_pk_write_raw, selector_bits=selector_bits,
                           num_selectors=num_selectors)

    def serialized_size(self, format: int = SERDE_PROCESSED, num_selectors: int = 0) -> int:
        return self.ctx.lib.cq_pk_serialized_size(self.h, format, num_selectors)

    def vk_commitments(self):
        """(fixed_commitments, permutation commitments) of the matching verifying key: uint64[.,8] affine points
        (keygen.rs:247-250, permutation/keygen.rs:115-149)."""
        nf = self.cs.num_fixed_columns if self.cs is not None else 0
        npc = len(self.cs.permutation_columns) if self.cs is not None else 0
        f = np.zeros((max(nf, 1), 8), dtype=np.uint64)
        p = np.zeros((max(npc, 1), 8), dtype=np.uint64)
        self.ctx._chk(self.ctx.lib.cq_pk_vk_commitments(self.h, f.ctypes.data, p.ctypes.data))
        return f[:nf], p[:npc]

    def b_row_bases(self, which):
        return self.ctx.lib.cq_pk_b_row_bases_dev(self.h, which)

    # ---- plonk/prover.rs: create_proof ----
    def set_opener(self, name: str):
        """`P: Prover` of create_proof: "gwc" (ProverGWC, default) or "shplonk" (ProverSHPLONK)."""
        self.ctx._chk(self.ctx.lib.cq_pk_set_opener(self.h, _OPENERS[name]))
        self.proof_size = self.ctx.lib.cq_pk_proof_size(self.h)

    def set_rng_fill(self, name):
        """cq_pk_set_rng_fill: None (per-word callbacks) or "opaque" (the harness generator's bulk form)."""
        fn = C.cast(self.ctx.lib.cq_opaque_rng_fill, C.c_void_p) if name == "opaque" else None
        self.ctx._chk(self.ctx.lib.cq_pk_set_rng_fill(self.h, fn))

    def _rng(self, rng_words=None, seed=None, opaque=False):
        lib = self.ctx.lib
        if rng_words is not None:
            w = np.ascontiguousarray(rng_words, dtype=np.uint64)
            st = _BufferRng(w.ctypes.data_as(C.POINTER(C.c_uint64)), 0, w.shape[0], 0)
            self._rng_keep = (w, st)
            return C.cast(lib.cq_buffer_rng_next_u64, C.c_void_p), C.cast(C.byref(st), C.c_void_p)
        st = (C.c_uint64 * 4)()
        lib.cq_xoshiro256ss_seed(seed, st)
        self._rng_keep = st
        # opaque: the same generator behind a function pointer the library does not recognise (a caller's RngCore)
        return C.cast(lib.cq_opaque_rng_next_u64 if opaque else lib.cq_xoshiro256ss_next_u64, C.c_void_p), C.cast(st, C.c_void_p)

    def _run(self, fn, ptrs, rng_fn, rng_state, instances=None, on_device=False) -> bytes:
        arr, out = _ptr_array(ptrs, False), _ProofBuffer(self.proof_size)
        if instances is None:
            self.ctx._chk(fn(self.h, arr, rng_fn, rng_state, *out.args))
        else:
            iptr, ilen, keep = _instance_columns(instances)
            self.ctx._chk(self.ctx.lib.cq_create_proof_instances(self.h, arr, 1 if on_device else 0, iptr, ilen, rng_fn, rng_state,
                                                                 *out.args))
            del keep
        return out.bytes()

    def create_proof(self, advice, rng_words=None, seed=None, instances=None) -> bytes:
        """`create_proof` (plonk/prover.rs:51) with host advice columns (uint64[n,4] each; rows
        beyond the usable rows are ignored) and public inputs `instances` (uint64[len,4] per instance
        column).  RNG: a pre-drawn u64 stream or a xoshiro256** seed."""
        cols = [np.ascontiguousarray(a, dtype=np.uint64) for a in advice]
        assert len(cols) == self.num_advice and all(c.shape == (1 << self.k, 4) for c in cols)
        fn, st = self._rng(rng_words, seed)
        return self._run(self.ctx.lib.cq_create_proof_host, [c.ctypes.data for c in cols], fn, st, instances)

    def create_proof_dev(self, advice_ptrs, rng_words=None, seed=None, instances=None, opaque_rng=False) -> bytes:
        fn, st = self._rng(rng_words, seed, opaque_rng)
        return self._run(self.ctx.lib.cq_create_proof, list(advice_ptrs), fn, st, instances, on_device=True)

    def create_proof_assigned(self, columns, rng_words=None, seed=None, instances=None) -> bytes:
        """`create_proof` from the `WitnessCollection` hand-over (plonk/prover.rs:337-360): `columns` are
        plonk.AssignedColumn objects of 2^k rows; batch_invert_assigned runs on the GPU (cq_create_proof_assigned)."""
        columns = list(columns)
        assert len(columns) == self.num_advice and all(c.n == 1 << self.k for c in columns)
        fn, st = self._rng(rng_words, seed)
        iptr, ilen, keep = _instance_columns(instances)
        out = _ProofBuffer(self.proof_size)
        self.ctx._chk(self.ctx.lib.cq_create_proof_assigned(self.h, _assigned_structs(columns), iptr, ilen, fn, st, *out.args))
        del keep
        return out.bytes()

    def create_proof_phases(self, advice_bufs, phase_fn, rng_words=None, seed=None, instances=None) -> bytes:
        """Multi-phase circuits (prover.rs:436-463): `advice_bufs` are DevBufs of 2^k elements; before phase p > 0 is
        committed `phase_fn(p, challenges)` is called with the user challenges so far (Python ints, canonical) and
        returns {advice column index: uint64[usable_rows.., 4] Montgomery limbs} for the columns of that phase."""
        fn, st = self._rng(rng_words, seed)
        nch = len(self.cs.challenge_phase)

        def _cb(_user, phase, ch_ptr, _adv):
            try:
                raw = np.ctypeslib.as_array(ch_ptr, shape=(max(nch, 1), 4))
                chal = [fr_from_mont(raw[i]) for i in range(nch)]
                for col, vals in phase_fn(phase, chal).items():
                    advice_bufs[col].upload(_fr(vals))
                return 0
            except Exception:  # the C side maps a non-zero status to CQ_ERR_ARG
                import traceback

                traceback.print_exc()
                return 1

        cb = _PHASE_T(_cb)
        iptr, ilen, keep = _instance_columns(instances or [])
        out = _ProofBuffer(self.proof_size)
        self.ctx._chk(self.ctx.lib.cq_create_proof_phases(self.h, _ptr_array([b.ptr for b in advice_bufs], False), iptr, ilen, cb, None,
                                                          fn, st, *out.args))
        del keep
        return out.bytes()

    def create_proof_batch(self, advice_ptr_lists, seeds, lanes: int = 0, opaque_rng: bool = False):
        """cq_create_proof_batch: one proof per entry of `advice_ptr_lists` (each a list of num_advice device pointers), blinded
        from xoshiro256** streams seeded with `seeds[i]`; returns the list of proofs."""
        lib = self.ctx.lib
        B = len(advice_ptr_lists)
        assert len(seeds) == B
        cols = [_ptr_array(p, False) for p in advice_ptr_lists]
        states = [(C.c_uint64 * 4)() for _ in range(B)]
        for st, sd in zip(states, seeds):
            lib.cq_xoshiro256ss_seed(sd, st)
        bufs = [(C.c_uint8 * self.proof_size)() for _ in range(B)]
        adv, st_arr, out = (_ptr_array([C.cast(x, C.c_void_p) for x in xs], False) for xs in (cols, states, bufs))
        lens = (C.c_size_t * max(B, 1))()
        fn = C.cast(lib.cq_opaque_rng_next_u64 if opaque_rng else lib.cq_xoshiro256ss_next_u64, C.c_void_p)
        self.ctx._chk(lib.cq_create_proof_batch(self.h, B, adv, fn, st_arr, out, self.proof_size, lens, lanes))
        return [bytes(bufs[i][: lens[i]]) for i in range(B)]

    # ---- plonk/static_lookup/prover.rs, plonk/evaluation.rs: the CQ rounds on their own ----
    def _shape(self):
        L = len(self.cs.static_lookups) if self.cs is not None else self._num_lookups
        return L, 1 << self.k, self._table_size

    def cq_round1(self, advice_ptrs, theta, instance_ptrs=None, challenges=None):
        """`static_lookup::Argument::commit` (static_lookup/prover.rs:51-183) on its own (cq_cq_round1_dev): returns
        (f DevBuf [L x n], m DevBuf [L x N uint32], commitments uint64[L, 2, 8] = (f_cm, m_cm) per lookup)."""
        L, n, N = self._shape()
        ctx = self.ctx
        f, m = ctx.alloc(max(L * n * 32, 32)), ctx.alloc(max(L * N * 4, 32))
        ch = np.ascontiguousarray(challenges, dtype=np.uint64) if challenges is not None else None
        cm = np.zeros((max(L, 1), 2, 8), dtype=np.uint64)
        ctx._chk(ctx.lib.cq_cq_round1_dev(self.h, _ptr_array(advice_ptrs, False), _ptr_array(instance_ptrs, True),
                                          ch.ctypes.data if ch is not None else None, _limbs4(theta).ctypes.data, f.ptr, m.ptr,
                                          cm.ctypes.data))
        return f, m, cm[:L]

    def cq_round2(self, f: DevBuf, m: DevBuf, theta, beta):
        """`Committed::commit_log_derivatives` (static_lookup/prover.rs:187-342) on its own (cq_cq_round2_dev): returns
        (b_coeff DevBuf, f_coeff DevBuf, commitments uint64[L, 5, 8] = (a, q_a, a_0, b_0, p), a_at_zero uint64[L, 4])."""
        L, n, _ = self._shape()
        ctx = self.ctx
        b, fc = ctx.alloc(max(L * n * 32, 32)), ctx.alloc(max(L * n * 32, 32))
        cm = np.zeros((max(L, 1), 5, 8), dtype=np.uint64)
        a0 = np.zeros((max(L, 1), 4), dtype=np.uint64)
        ctx._chk(ctx.lib.cq_cq_round2_dev(self.h, f.ptr, m.ptr, _limbs4(theta).ctypes.data, _limbs4(beta).ctypes.data, b.ptr, fc.ptr,
                                          cm.ctypes.data, a0.ctypes.data))
        return b, fc, cm[:L], a0[:L]

    def cq_quotient(self, b_coeff: DevBuf, f_coeff: DevBuf, y, beta, h_in: DevBuf = None, divide: bool = True, ext: int = None) -> DevBuf:
        """The static-lookup terms of `Evaluator::evaluate_h` (evaluation.rs:533-548), optionally followed by
        `divide_by_vanishing_poly` (domain.rs:319-338) (cq_quotient_dev); `ext` = 2^extended_k elements come back."""
        ctx = self.ctx
        out = ctx.alloc(ext * 32)
        ctx._chk(ctx.lib.cq_quotient_dev(self.h, b_coeff.ptr, f_coeff.ptr, _limbs4(y).ctypes.data, _limbs4(beta).ctypes.data,
                                         h_in.ptr if h_in else None, 1 if divide else 0, out.ptr))
        return out

    # ---- plonk/permutation/prover.rs, plonk/lookup/prover.rs, plonk/evaluation.rs, poly/kzg/multiopen: the other stages ----
    def permutation_commit(self, advice_ptrs, beta, gamma, instance_ptrs=None, rng_words=None, seed=None, rng=None):
        """`permutation::Argument::commit` (permutation/prover.rs:47-198) on its own (cq_permutation_commit_dev): the columns
        are device pointers to n Lagrange values (blinding rows included); returns (z DevBuf [sets x n coefficients],
        commitments uint64[sets, 8]).  RNG: a pre-drawn u64 stream, a xoshiro256** seed, or `rng` = the (function, state) pair
        of an earlier `_rng` call to go on drawing from the same stream."""
        ctx, n = self.ctx, 1 << self.k
        if len(list(advice_ptrs)) != self.num_advice:
            raise CqError(-1, f"permutation_commit: the key has {self.num_advice} advice columns, {len(list(advice_ptrs))} given")
        sets = ctx.lib.cq_pk_permutation_sets(self.h)  # the key's own count sizes the outputs
        z = ctx.alloc(max(sets * n * 32, 32))
        cm = np.zeros((max(sets, 1), 8), dtype=np.uint64)
        fn, st = rng if rng is not None else self._rng(rng_words, seed)
        ctx._chk(ctx.lib.cq_permutation_commit_dev(self.h, _ptr_array(advice_ptrs, True), _ptr_array(instance_ptrs, True),
                                                   _limbs4(beta).ctypes.data, _limbs4(gamma).ctypes.data, fn, st, z.ptr, cm.ctypes.data))
        return z, cm[:sets]

    def lookup_commit_product(self, input_ptrs, table_ptrs, permuted_input_ptrs, permuted_table_ptrs, beta, gamma, rng_words=None,
                              seed=None, rng=None):
        """`lookup::Permuted::commit_product` (lookup/prover.rs:173-318) for every legacy lookup of the key
        (cq_lookup_commit_product_dev): per lookup the compressed input / table and the permuted pair (blinding rows appended),
        device pointers to n Lagrange values; returns (z DevBuf [lookups x n coefficients], commitments uint64[lookups, 8])."""
        ctx, n = self.ctx, 1 << self.k
        PL = ctx.lib.cq_pk_legacy_lookups(self.h)
        for ptrs in (input_ptrs, table_ptrs, permuted_input_ptrs, permuted_table_ptrs):
            if len(list(ptrs)) != PL:
                raise CqError(-1, f"lookup_commit_product: the key has {PL} legacy lookups, {len(list(ptrs))} columns given")
        z = ctx.alloc(max(PL * n * 32, 32))
        cm = np.zeros((max(PL, 1), 8), dtype=np.uint64)
        fn, st = rng if rng is not None else self._rng(rng_words, seed)
        ctx._chk(ctx.lib.cq_lookup_commit_product_dev(self.h, _ptr_array(input_ptrs, True), _ptr_array(table_ptrs, True),
                                                      _ptr_array(permuted_input_ptrs, True), _ptr_array(permuted_table_ptrs, True),
                                                      _limbs4(beta).ctypes.data, _limbs4(gamma).ctypes.data, fn, st, z.ptr,
                                                      cm.ctypes.data))
        return z, cm[:PL]

    def evaluate_h(self, advice_coeff_ptrs, beta, gamma, theta, y, ext: int, instance_coeff_ptrs=None, perm_z: DevBuf = None,
                   permuted_input_coeff_ptrs=None, permuted_table_coeff_ptrs=None, lookup_z: DevBuf = None, challenges=None) -> DevBuf:
        """The gates, permutation terms and legacy-lookup terms of `Evaluator::evaluate_h` (evaluation.rs:285-531) on the
        extended coset (cq_evaluate_h_dev): all polynomials in coefficient form on the device; the `ext` elements that come
        back are `cq_quotient`'s `h_in`."""
        ctx = self.ctx
        out = ctx.alloc(ext * 32)
        ch = np.ascontiguousarray(challenges, dtype=np.uint64) if challenges is not None else None
        ctx._chk(ctx.lib.cq_evaluate_h_dev(self.h, _ptr_array(advice_coeff_ptrs, True), _ptr_array(instance_coeff_ptrs, True),
                                           perm_z.ptr if perm_z else None, _ptr_array(permuted_input_coeff_ptrs, True),
                                           _ptr_array(permuted_table_coeff_ptrs, True), lookup_z.ptr if lookup_z else None,
                                           ch.ctypes.data if ch is not None else None, _limbs4(beta).ctypes.data,
                                           _limbs4(gamma).ctypes.data, _limbs4(theta).ctypes.data, _limbs4(y).ctypes.data, out.ptr))
        return out

    def multiopen(self, queries, squeeze_challenge, write_point):
        """The multi-open argument with the key's opener (`set_opener`) for arbitrary queries (cq_multiopen_dev): `queries`
        = [(device pointer, length <= n, point uint64[4])]; `squeeze_challenge()` returns the next challenge as Montgomery
        limbs uint64[4], `write_point(affine uint64[8])` takes a commitment.  An exception in either fails the call."""
        ctx = self.ctx
        qs = (_CqOpenQuery * max(len(queries), 1))()
        for i, (ptr, length, point) in enumerate(queries):
            qs[i] = _struct_of(_CqOpenQuery, ptr, length, tuple(int(limb) for limb in _limbs4(point)))

        def _squeeze(_user, out):
            try:
                for i, limb in enumerate(_limbs4(squeeze_challenge())):
                    out[i] = int(limb)
                return 0
            except Exception:  # the C side maps a non-zero status to CQ_ERR_ARG
                return 1

        def _write(_user, affine):
            try:
                write_point(np.array([affine[i] for i in range(8)], dtype=np.uint64))
                return 0
            except Exception:
                return 1

        sq, wr = _SQUEEZE_T(_squeeze), _WRITE_POINT_T(_write)
        tr = _CqOpenTranscript(C.cast(sq, C.c_void_p), C.cast(wr, C.c_void_p), None)
        ctx._chk(ctx.lib.cq_multiopen_dev(self.h, qs, len(queries), C.byref(tr)))

    # ---- dev.rs: MockProver ----
    def check_witness(self, advice, instances=None, challenges=None, max_failures=64):
        """`MockProver::verify` (dev.rs:601-958) on the GPU, static lookups included (cq_pk_check_witness): checks the
        witness `create_proof*` would be given against the key and returns `(total, [WitnessFailure, ...])` -- the exact
        number of findings and the first `max_failures` of them in ascending (kind, index, row) order.  `advice`: every
        advice column of every phase, as host arrays (uint64[n, 4]), as device pointers (ints / DevBufs) or as
        plonk.AssignedColumn objects (resolved first by cq_batch_invert_assigned_dev); `instances`
        as for create_proof; `challenges`: the user challenges the later phases were synthesised with (Python ints,
        canonical, or uint64[4] Montgomery limbs each)."""
        resolved = None
        if len(advice) > 0 and all(hasattr(a, "den_rows") for a in advice):  # plonk.AssignedColumn: resolved on the GPU first
            advice = resolved = self.ctx._resolve_assigned_to_device(advice)
        on_device = len(advice) > 0 and all(isinstance(a, (int, DevBuf)) for a in advice)
        if on_device:
            ptrs = [a.ptr if isinstance(a, DevBuf) else a for a in advice]
        else:
            cols = [np.ascontiguousarray(a, dtype=np.uint64) for a in advice]
            assert all(c.shape == (1 << self.k, 4) for c in cols), "advice columns are uint64[2^k, 4]"
            ptrs = [c.ctypes.data for c in cols]
        assert len(ptrs) == self.num_advice
        iptr, ilen, keep = _instance_columns(instances)
        ch_ptr = None
        if challenges is not None and len(challenges):
            ch = np.stack([fr_to_mont(int(v)) if np.ndim(v) == 0 else _limbs4(v) for v in challenges])
            ch = np.ascontiguousarray(ch, dtype=np.uint64)
            ch_ptr = ch.ctypes.data
        cap = max(int(max_failures), 0)
        out = np.zeros((max(cap, 1), 4), dtype=np.uint32)
        total = C.c_size_t()
        try:
            self.ctx._chk(self.ctx.lib.cq_pk_check_witness(self.h, _ptr_array(ptrs, False), 1 if on_device else 0, iptr, ilen, ch_ptr,
                                                           out.ctypes.data if cap else None, cap, C.byref(total)))
        finally:
            for b in resolved or []:
                b.free()
        del keep
        return total.value, [WitnessFailure(*(int(x) for x in row)) for row in out[: min(cap, total.value)]]

    def assert_satisfied(self, advice, instances=None, challenges=None, max_failures=8):
        """`MockProver::assert_satisfied` (dev.rs:960-990): raises `WitnessError` (a `CqError`) naming the first failures."""
        total, fails = self.check_witness(advice, instances, challenges, max_failures)
        if total:
            raise WitnessError(total, fails)

    # ---- no counterpart in the reference: one proof sharded across the ranks of a job ----
    def _install_sharding(self, rank: int, world: int, columns: bool, resident: bool, allgather=None, bcast=None, exchange=None):
        # the library keeps the addresses of the callback objects: the ones it held so far stay referenced (`old`) until it
        # has been given the new ones, which live on the key
        old = self.__dict__.get("_allgather_cb"), self.__dict__.get("_bcast_cb"), self.__dict__.get("_exchange_cb")
        self._allgather_cb, self._bcast_cb, self._exchange_cb = allgather, bcast, exchange
        lib, hook = self.ctx.lib, lambda cb: C.cast(cb, C.c_void_p) if cb is not None else None
        self.ctx._chk(lib.cq_pk_set_resident_sharding(self.h, 1 if resident else 0, hook(exchange), None))
        self.ctx._chk(lib.cq_pk_set_column_sharding(self.h, 1 if columns else 0, hook(bcast), None))
        self.ctx._chk(lib.cq_pk_set_sharding(self.h, rank, world, hook(allgather), None))
        del old

    def set_sharding(self, rank: int, world: int, group=None, device=None, transport: str = "callback", columns: bool = True,
                     resident: bool = False):
        """Shards `create_proof` across the ranks of a job (cq_pk_set_sharding + cq_pk_set_column_sharding): every
        commitment by point range (all-gather of the per-rank Jacobian partials) and, with `columns`, the independent column
        transforms by owner (broadcast of the transformed columns).
        transport "rccl": the library's own ncclAllGather / ncclBroadcast on device buffers, on the context's communicator
        (Context.comm_init_rccl / comm_init_from_torch first); "callback": torch.distributed collectives of `group` on host
        buffers (gloo on CPU tensors; with `device` the tensors travel through that device for the "nccl" backend).
        `resident`: cq_pk_set_resident_sharding -- transformed columns stay on their owner and slices travel point to point
        (ncclSend / ncclRecv, or torch.distributed isend / irecv on host buffers)."""
        if world <= 1:
            return self._install_sharding(0, 1, columns, resident)
        if transport == "rccl":
            return self._install_sharding(rank, world, columns, resident)
        import torch
        import torch.distributed as dist

        def allgather(_user, send, recv, nbytes):
            try:
                src = (C.c_uint8 * nbytes).from_address(send)
                t = torch.frombuffer(src, dtype=torch.uint8).clone()
                if device is not None:
                    t = t.to(device)
                outs = [torch.empty_like(t) for _ in range(world)]
                dist.all_gather(outs, t, group=group)
                dst = (C.c_uint8 * (nbytes * world)).from_address(recv)
                flat = torch.cat([o.cpu() for o in outs]).numpy()
                C.memmove(dst, flat.ctypes.data, nbytes * world)
                return 0
            except Exception:  # never unwind into C
                return -1

        def bcast(_user, buf, nbytes, root):
            try:
                mem = (C.c_uint8 * nbytes).from_address(buf)
                t = torch.frombuffer(mem, dtype=torch.uint8)  # shares the library's host buffer
                if device is not None:
                    d = t.to(device)
                    dist.broadcast(d, src=dist.get_global_rank(group, root) if group is not None else root, group=group)
                    t.copy_(d.cpu())
                else:
                    dist.broadcast(t, src=dist.get_global_rank(group, root) if group is not None else root, group=group)
                return 0
            except Exception:
                return -1

        def exchange(_user, xfers, count):
            try:
                ops, keep = [], []
                for i in range(count):
                    x = xfers[i]
                    mem = (C.c_uint8 * x.bytes).from_address(x.buf)
                    t = torch.frombuffer(mem, dtype=torch.uint8)  # shares the library's host buffer
                    peer = dist.get_global_rank(group, x.peer) if group is not None else x.peer
                    if device is not None:
                        d = t.to(device) if x.send else torch.empty(x.bytes, dtype=torch.uint8, device=device)
                        keep.append((None if x.send else t, d))
                        ops.append(dist.P2POp(dist.isend if x.send else dist.irecv, d, peer, group))
                    else:
                        ops.append(dist.P2POp(dist.isend if x.send else dist.irecv, t, peer, group))
                for req in dist.batch_isend_irecv(ops):
                    req.wait()
                for t, d in keep:
                    if t is not None:
                        t.copy_(d.cpu())
                return 0
            except Exception:
                import traceback

                traceback.print_exc()
                return -1

        self._install_sharding(rank, world, columns, resident, _ALLGATHER_T(allgather), _BCAST_T(bcast), _EXCHANGE_T(exchange))

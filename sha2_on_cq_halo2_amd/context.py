"""`Context` -- one GPU, one stream, and the reference's free functions (halo2_proofs/src/arithmetic.rs and friends) as its
methods -- with the two kinds of object a context owns: device buffers (`DevBuf`) and library handles (`_Handle`).

Names, argument meaning and error behaviour follow the Rust functions they stand for; contract violations that panic in
Rust raise `CqError` here.
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from ._lib import CqError, load
from ._marshal import (RCCL_UNIQUE_ID_BYTES, _CqAssignedColumn, _assigned_structs, _fr, _fr_or_empty, _g1, _g2, _limbs4,
                       _ptr_array, _struct_of)


class DevBuf:
    """Device allocation owned by a Context."""

    _close_first = False

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx = ctx
        self.nbytes = nbytes
        p = C.c_void_p()
        ctx._chk(ctx.lib.cq_dev_alloc(ctx.h, nbytes, C.byref(p)))
        self.ptr = p.value
        ctx._children.add(self)

    def upload(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.ctx._chk(self.ctx.lib.cq_dev_upload(self.ctx.h, self.ptr, arr.ctypes.data, arr.nbytes))
        return self

    def download(self, shape, dtype=np.uint64) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        self.ctx._chk(self.ctx.lib.cq_dev_download(self.ctx.h, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr and self.ctx.h:
            self.ctx.lib.cq_dev_free(self.ctx.h, self.ptr)
        self.ptr = None

    close = free

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _Handle:
    """An object of the library that lives on a context: params, domains, tables, keys."""

    _destroy = None        # the entry point that frees the handle
    _close_first = False   # Context.close closes these before the rest (a key refers to what it was built on)

    def _open(self, ctx: "Context", create, *args):
        """`create(*args, &handle)`: checks the status, keeps the handle and registers the object with its context."""
        h = C.c_void_p()
        ctx._chk(create(*args, C.byref(h)))
        self.ctx, self.h = ctx, h
        ctx._children.add(self)
        return self

    def close(self):
        if self.h and self.ctx.h:
            getattr(self.ctx.lib, self._destroy)(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _host_or_device_points(points, need: int):
    """(address, on_device, keep-alive) of G1 points given as a uint64[n,8] host array (n >= need), a DevBuf or a device
    address."""
    if isinstance(points, DevBuf):
        return points.ptr, 1, points
    if isinstance(points, (int, np.integer)):
        return int(points), 1, None
    a = _g1(points)
    if a.shape[0] < need:
        raise CqError(-1, "fewer points than the object needs")
    return a.ctypes.data, 0, a


def rccl_unique_id() -> bytes:
    """cq_rccl_unique_id: drawn by ONE rank and handed to the others (e.g. with a torch.distributed broadcast)."""
    buf = (C.c_uint8 * RCCL_UNIQUE_ID_BYTES)()
    rc = load().cq_rccl_unique_id(buf)
    if rc != 0:
        raise CqError(rc, "cq_rccl_unique_id failed (librccl not loadable?)")
    return bytes(buf)


class Context:
    def __init__(self, device: int = 0, stream: int | None = None):
        self.lib = load()
        h = C.c_void_p()
        rc = self.lib.cq_ctx_create(device, stream, C.byref(h))
        if rc != 0:
            raise CqError(rc, "cq_ctx_create failed (no usable GPU?)")
        self.h = h
        self._children = weakref.WeakSet()  # device objects that must die before the context

    def close(self):
        if self.h:
            # proving keys first: a key refers to the params / table config it was built on until it is destroyed
            for ch in sorted(list(self._children), key=lambda o: not o._close_first):
                ch.close()
            self.lib.cq_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int):
        if rc != 0:
            raise CqError(rc, self.lib.cq_last_error(self.h).decode())

    def sync(self):
        self._chk(self.lib.cq_ctx_sync(self.h))

    @property
    def stream(self) -> int:
        return self.lib.cq_ctx_stream(self.h)

    def alloc(self, nbytes: int) -> DevBuf:
        return DevBuf(self, nbytes)

    def to_device(self, arr: np.ndarray) -> DevBuf:
        arr = np.ascontiguousarray(arr)
        return DevBuf(self, max(arr.nbytes, 1)).upload(arr)

    def set_hip_graphs(self, on):
        self._chk(self.lib.cq_ctx_set_hip_graphs(self.h, 1 if on else 0))

    # ---- arithmetic.rs: best_fft, eval_polynomial, kate_division, batch_invert ----
    def best_fft(self, a: np.ndarray, omega: np.ndarray, log_n: int) -> np.ndarray:
        """`best_fft(a, omega, log_n)` (arithmetic.rs:171): returns the transformed copy."""
        a = _fr(a).copy()
        if a.shape[0] != 1 << log_n:  # arithmetic.rs:184 assert
            raise CqError(-1, "best_fft: len != 1 << log_n")
        self._chk(self.lib.cq_best_fft(self.h, a.ctypes.data, log_n, _limbs4(omega).ctypes.data))
        return a

    def best_fft_dev(self, src: DevBuf, dst: DevBuf, omega: np.ndarray, log_n: int):
        self._chk(self.lib.cq_best_fft_dev(self.h, src.ptr, dst.ptr, log_n, _limbs4(omega).ctypes.data))

    def eval_polynomial(self, poly: np.ndarray, point: np.ndarray) -> np.ndarray:
        """`eval_polynomial(poly, point)` (arithmetic.rs:304)."""
        poly = _fr_or_empty(poly)
        out = np.zeros(4, dtype=np.uint64)
        self._chk(self.lib.cq_eval_polynomial(self.h, poly.ctypes.data, poly.shape[0], _limbs4(point).ctypes.data, out.ctypes.data))
        return out

    def kate_division(self, a: np.ndarray, b: np.ndarray) -> np.ndarray:
        """`kate_division(a, b)` (arithmetic.rs:351): n-1 quotient coefficients."""
        a = _fr(a)
        q = np.zeros((max(a.shape[0] - 1, 0), 4), dtype=np.uint64)
        self._chk(self.lib.cq_kate_division(self.h, a.ctypes.data, a.shape[0], _limbs4(b).ctypes.data, q.ctypes.data))
        return q

    def batch_invert(self, a: np.ndarray) -> np.ndarray:
        """`BatchInvert::batch_invert` (ff 0.12): returns the inverted copy, zeros untouched."""
        a = _fr(a).copy() if len(a) else np.zeros((0, 4), dtype=np.uint64)
        self._chk(self.lib.cq_batch_invert(self.h, a.ctypes.data, a.shape[0]))
        return a

    # ---- arithmetic.rs: best_multiexp and its knobs ----
    def _multiexp(self, fn, points, width: int, coeffs: np.ndarray, bases: np.ndarray) -> np.ndarray:
        coeffs = _fr_or_empty(coeffs)
        bases = points(bases) if len(bases) else np.zeros((0, width), dtype=np.uint64)
        if coeffs.shape[0] != bases.shape[0]:  # arithmetic.rs:133 assert_eq
            raise CqError(-1, "best_multiexp: coeffs.len() != bases.len()")
        out = np.zeros(3 * width // 2, dtype=np.uint64)
        self._chk(fn(self.h, coeffs.ctypes.data, bases.ctypes.data, coeffs.shape[0], out.ctypes.data))
        return out

    def best_multiexp(self, coeffs: np.ndarray, bases: np.ndarray) -> np.ndarray:
        """`best_multiexp(coeffs, bases)` (arithmetic.rs:132): Jacobian result, uint64[12]."""
        return self._multiexp(self.lib.cq_best_multiexp, _g1, 8, coeffs, bases)

    def best_multiexp_g2(self, coeffs: np.ndarray, bases: np.ndarray) -> np.ndarray:
        """`best_multiexp(coeffs, bases)` over G2Affine (arithmetic.rs:132): Jacobian result, uint64[24]."""
        return self._multiexp(self.lib.cq_best_multiexp_g2, _g2, 16, coeffs, bases)

    def best_multiexp_dev(self, coeffs: DevBuf, bases: DevBuf, n: int) -> np.ndarray:
        out = np.zeros(12, dtype=np.uint64)
        self._chk(self.lib.cq_best_multiexp_dev(self.h, coeffs.ptr, bases.ptr, n, out.ctypes.data))
        return out

    def best_multiexp_g2_dev(self, coeffs: DevBuf, bases_ptr: int, n: int) -> np.ndarray:
        out = np.zeros(24, dtype=np.uint64)
        self._chk(self.lib.cq_best_multiexp_g2_dev(self.h, coeffs.ptr, bases_ptr, n, out.ctypes.data))
        return out

    def msm_batch_dev(self, coeff_ptrs, bases_ptr: int, n: int) -> np.ndarray:
        out = np.zeros((len(coeff_ptrs), 12), dtype=np.uint64)
        self._chk(self.lib.cq_msm_batch_dev(self.h, _ptr_array(coeff_ptrs, False), bases_ptr, n, len(coeff_ptrs), out.ctypes.data))
        return out

    def msm_bucket_sums(self, bases_ptrs, index: np.ndarray, buckets: int, packed: bool = False) -> np.ndarray:
        """cq_msm_bucket_sums_dev: out[a, b] = the sum of the points bases_ptrs[a][i] with index[i] == b (affine, uint64[arrays,
        buckets, 8]; the identity for an empty bucket).  `packed`: the arrays are ProvingKey.b_row_bases pointers."""
        idx = self.to_device(np.ascontiguousarray(index, dtype=np.uint32))
        out = self.alloc(len(bases_ptrs) * buckets * 64)
        try:
            self._chk(self.lib.cq_msm_bucket_sums_dev(self.h, _ptr_array(bases_ptrs, False), len(bases_ptrs), 1 if packed else 0, idx.ptr,
                                                      len(index), buckets, out.ptr))
            return out.download((len(bases_ptrs), buckets, 8))
        finally:
            idx.close()
            out.close()

    def set_msm_window(self, bits: int):
        self._chk(self.lib.cq_msm_set_window(self.h, bits))

    def set_msm_table_window(self, bits: int):
        """Window width of the per-window tables built from now on (8..20, 0 = automatic); see cq_msm_set_table_window."""
        self._chk(self.lib.cq_msm_set_table_window(self.h, bits))

    def msm_precompute(self, bases_ptr: int, n: int):
        """Registers per-window tables for a device-resident base array (fixed-base acceleration)."""
        self._chk(self.lib.cq_msm_precompute_dev(self.h, bases_ptr, n))

    def set_msm_precompute(self, on: bool):
        self._chk(self.lib.cq_msm_set_precompute(self.h, 1 if on else 0))

    def msm_table_width(self, bases_ptr: int, n: int, preferred: int = 0) -> int:
        """Window width of the precomputed tables a multiexp over [bases_ptr, bases_ptr + n) would use (0: none)."""
        bits = C.c_uint32()
        self._chk(self.lib.cq_msm_table_width_dev(self.h, bases_ptr, n, preferred, C.byref(bits)))
        return bits.value

    # ---- arithmetic.rs: g_to_lagrange ----
    def _g_to_lagrange(self, fn, points: np.ndarray, k: int) -> np.ndarray:
        g = _g1(points)
        if g.shape[0] != 1 << k:
            raise CqError(-1, "g_to_lagrange: len != 1 << k")
        dg, out = self.to_device(g), self.alloc(g.shape[0] * 64)
        self._chk(fn(self.h, dg.ptr, k, out.ptr))
        return out.download((g.shape[0], 8), np.uint64)

    def g_to_lagrange(self, points: np.ndarray, k: int) -> np.ndarray:
        """`g_to_lagrange(g_projective, k)` (arithmetic.rs:277-301) on the device: 2^k affine points in, the Lagrange-basis
        points out (uint64[2^k, 8]).  Any points, the identity (0, 0) included; nothing is validated."""
        return self._g_to_lagrange(self.lib.cq_g_to_lagrange_dev, points, k)

    def g_to_lagrange_windowed(self, points: np.ndarray, k: int) -> np.ndarray:
        """`g_to_lagrange` by the fixed-window G1 FFT of the trapdoor-free setup path: the same bytes as `g_to_lagrange`."""
        return self._g_to_lagrange(self.lib.cq_g_to_lagrange_windowed_dev, points, k)

    # ---- poly.rs: batch_invert_assigned ----
    def batch_invert_assigned(self, columns):
        """`batch_invert_assigned` (poly.rs:212-241) on plonk.AssignedColumn objects of one length: the resolved columns,
        uint64[n, 4] each (cq_batch_invert_assigned)."""
        columns = list(columns)
        if not columns:
            return []
        n = columns[0].n
        assert all(c.n == n for c in columns), "columns of one length"
        out = [np.zeros((n, 4), dtype=np.uint64) for _ in columns]
        optr = _ptr_array([o.ctypes.data for o in out], False)
        self._chk(self.lib.cq_batch_invert_assigned(self.h, _assigned_structs(columns), len(columns), n, optr))
        return out

    def batch_invert_assigned_dev(self, columns, n: int, out_ptrs):
        """cq_batch_invert_assigned_dev: `columns` = (num_ptr, den_rows_ptr, den_ptr, den_count) of device arrays per column,
        `out_ptrs` the device outputs (may be the numerator arrays)."""
        arr = (_CqAssignedColumn * max(len(columns), 1))(*[_struct_of(_CqAssignedColumn, *c) for c in columns])
        self._chk(self.lib.cq_batch_invert_assigned_dev(self.h, arr, len(columns), n, _ptr_array(out_ptrs, False)))

    def _resolve_assigned_to_device(self, columns):
        """Uploads plonk.AssignedColumn objects and resolves them in place through the device entry point: one DevBuf each."""
        bufs, keep, descr = [], [], []
        for col in columns:
            num = self.to_device(col.num)
            m = col.den_rows.shape[0]
            rows, den = (self.to_device(col.den_rows), self.to_device(col.den)) if m else (None, None)
            keep += [rows, den]
            bufs.append(num)
            descr.append((num.ptr, rows.ptr if m else None, den.ptr if m else None, m))
        if columns:
            self.batch_invert_assigned_dev(descr, columns[0].n, [b.ptr for b in bufs])
        for b in keep:
            if b is not None:
                b.free()
        return bufs

    # ---- plonk/lookup/prover.rs ----
    def permute_expression_pair(self, k: int, input_values: np.ndarray, table_values: np.ndarray):
        """`permute_expression_pair` (plonk/lookup/prover.rs:400-502) on the device, without the blinding rows: returns the
        permuted input and table (Montgomery limbs, `usable` rows each).  Raises on an input value the table does not hold."""
        a, t = _fr(input_values), _fr(table_values)
        assert a.shape == t.shape
        usable = a.shape[0]
        da, dt = self.to_device(a), self.to_device(t)
        oa, ot = self.alloc(usable * 32), self.alloc(usable * 32)
        self._chk(self.lib.cq_permute_expression_pair_dev(self.h, k, usable, da.ptr, dt.ptr, oa.ptr, ot.ptr))
        return oa.download((usable, 4), np.uint64), ot.download((usable, 4), np.uint64)

    # ---- derive/curve.rs, helpers.rs: the element conversions of the serialized formats, over device arrays ----
    def _checked_conversion(self, fn, src: DevBuf, n: int, dst: DevBuf):
        bad = C.c_size_t()
        rc = fn(self.h, src.ptr, n, dst.ptr, C.byref(bad))
        if rc != 0:
            e = CqError(rc, self.lib.cq_last_error(self.h).decode())
            e.first_bad = bad.value if rc == -1 else None
            raise e

    def g1_decompress(self, src: DevBuf, n: int, dst: DevBuf):
        """`CurveAffine::from_bytes` (derive/curve.rs:603-627) over a device array: n x 32 B -> n raw affine points.  An invalid
        encoding raises CqError whose `first_bad` is the lowest invalid index."""
        self._checked_conversion(self.lib.cq_g1_decompress_dev, src, n, dst)

    def g1_compress(self, src: DevBuf, n: int, dst: DevBuf):
        """`CurveAffine::to_bytes` (derive/curve.rs:635-646) over a device array: n raw affine points -> n x 32 B."""
        self._chk(self.lib.cq_g1_compress_dev(self.h, src.ptr, n, dst.ptr))

    def g2_decompress(self, src: DevBuf, n: int, dst: DevBuf):
        """`GroupEncoding::from_bytes` for G2Affine (derive/curve.rs:603-627) over a device array: n x 64 B -> n raw affine points
        (uint64[16] each).  An invalid encoding raises CqError whose `first_bad` is the lowest invalid index."""
        self._checked_conversion(self.lib.cq_g2_decompress_dev, src, n, dst)

    def g2_compress(self, src: DevBuf, n: int, dst: DevBuf):
        """`GroupEncoding::to_bytes` for G2Affine (derive/curve.rs:635-646) over a device array: n raw affine points -> n x 64 B."""
        self._chk(self.lib.cq_g2_compress_dev(self.h, src.ptr, n, dst.ptr))

    def fr_from_repr(self, src: DevBuf, n: int, dst: DevBuf):
        """`Fr::from_repr` (helpers.rs:68-79) over a device array: n x 32 B canonical little-endian -> Montgomery limbs (dst may be
        src).  A value >= r raises CqError whose `first_bad` is the lowest such index."""
        self._checked_conversion(self.lib.cq_fr_from_repr_dev, src, n, dst)

    def fr_to_repr(self, src: DevBuf, n: int, dst: DevBuf):
        """`Fr::to_repr` (helpers.rs:81-91) over a device array."""
        self._chk(self.lib.cq_fr_to_repr_dev(self.h, src.ptr, n, dst.ptr))

    # ---- sha/src/tables.rs ----
    def sha_synthesis_table(self, kind: int, first: int, second: int) -> np.ndarray:
        """`create_{rot0,rot1,maj,ch}_table::<L>` (sha/src/tables.rs:105-133): uint64[rows,4] = (x,y,z,f)."""
        rows = 1 << (first + 2 * second)
        buf = self.alloc(rows * 32)
        self._chk(self.lib.cq_sha_synthesis_table_dev(self.h, kind, first, second, buf.ptr))
        return buf.download((rows, 4))

    def sha_decomposition_table(self, first: int, second: int, k_bits: int) -> np.ndarray:
        """`create_decomposition_table::<L,K>` (sha/src/tables.rs:135-154): uint64[2^K,4] = (a,x,y,z)."""
        rows = 1 << k_bits
        buf = self.alloc(rows * 32)
        self._chk(self.lib.cq_sha_decomposition_table_dev(self.h, first, second, k_bits, buf.ptr))
        return buf.download((rows, 4))

    # ---- no counterpart in the reference: kernel timers, the RCCL communicator of sharded proving ----
    def profile_enable(self, on: bool = True):
        self._chk(self.lib.cq_profile_enable(self.h, 1 if on else 0))

    def profile_read(self, which: int):
        """(total milliseconds, launches) of the bracketed kernel since the last read."""
        ms = C.c_double()
        calls = C.c_uint64()
        self._chk(self.lib.cq_profile_read(self.h, which, C.byref(ms), C.byref(calls)))
        return ms.value, calls.value

    def comm_init_rccl(self, rank: int, world: int, unique_id: bytes):
        """cq_ctx_comm_init_rccl: the context's RCCL communicator (collective: every rank calls it with the same id)."""
        assert len(unique_id) == RCCL_UNIQUE_ID_BYTES
        buf = (C.c_uint8 * RCCL_UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        self._chk(self.lib.cq_ctx_comm_init_rccl(self.h, rank, world, buf))

    def comm_init_from_torch(self, device=None, group=None):
        """Convenience for torch.distributed jobs: rank 0 draws the RCCL id, the process group broadcasts it (a CUDA tensor
        over the "nccl" backend, a CPU tensor over gloo), every rank initialises the context's communicator."""
        import torch
        import torch.distributed as dist

        rank, world = dist.get_rank(group), dist.get_world_size(group)
        t = torch.zeros(RCCL_UNIQUE_ID_BYTES, dtype=torch.uint8)
        if rank == 0:
            t = torch.frombuffer(bytearray(rccl_unique_id()), dtype=torch.uint8).clone()
        if device is not None:
            t = t.to(device)
        dist.broadcast(t, src=0, group=group)
        self.comm_init_rccl(rank, world, bytes(t.cpu().numpy().tobytes()))

    def comm_destroy(self):
        self._chk(self.lib.cq_ctx_comm_destroy(self.h))

    def comm_selftest(self):
        self._chk(self.lib.cq_ctx_comm_selftest(self.h))

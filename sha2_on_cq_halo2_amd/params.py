"""The setup objects resident on the GPU: `ParamsKZG` and the G2 powers (poly/kzg/commitment.rs), the static-lookup table
objects (plonk/static_lookup.rs) and `EvaluationDomain` (poly/domain.rs)."""
from __future__ import annotations

import numpy as np

from ._lib import CqError
from ._marshal import SERDE_PROCESSED, _fr, _g1, _g2, _limbs4, _written
from .context import Context, DevBuf, _Handle, _host_or_device_points


class ParamsKZG(_Handle):
    """`ParamsKZG<Bn256>` (poly/kzg/commitment.rs:31-39): the G1 SRS resident on the GPU; g2 / s_g2 when the params were set up
    from toxic waste, read with `read_full` or given them with `set_g2`."""

    _destroy = "cq_params_destroy"

    def _open_k(self, k: int, ctx: Context, create, *args) -> "ParamsKZG":
        self.k, self.n = k, 1 << k
        return self._open(ctx, create, *args)

    # ---- kzg/commitment.rs: new, setup, downsize ----
    def __init__(self, ctx: Context, k: int, g: np.ndarray, g_lagrange: np.ndarray):
        g = _g1(g)
        g_lagrange = _g1(g_lagrange)
        assert g.shape[0] == 1 << k and g_lagrange.shape[0] == 1 << k
        self._open_k(k, ctx, ctx.lib.cq_params_create, ctx.h, k, g.ctypes.data, g_lagrange.ctypes.data)

    @classmethod
    def setup_from_toxic_waste(cls, ctx: Context, k: int, s: np.ndarray) -> "ParamsKZG":
        """`ParamsKZG::setup_from_toxic_waste(k, s)` (commitment.rs:209-276), built on the GPU."""
        return cls.__new__(cls)._open_k(k, ctx, ctx.lib.cq_params_setup_from_toxic_waste, ctx.h, k, _limbs4(s).ctypes.data)

    @classmethod
    def from_powers(cls, ctx: Context, k: int, g) -> "ParamsKZG":
        """`ParamsKZG` from the monomial powers [s^i]_1 alone, as a ceremony file holds them: g_lagrange is derived on the GPU
        (`g_to_lagrange`, arithmetic.rs:277-301).  `g`: uint64[2^k, 8] host array, or a device pointer (int / DevBuf) to 2^k
        affine points, which is copied.  No G2 tail (`set_g2`), as after `ParamsKZG(ctx, k, g, g_lagrange)`."""
        ptr, on_device, keep = _host_or_device_points(g, 1 << k)
        self = cls.__new__(cls)._open_k(k, ctx, ctx.lib.cq_params_from_powers, ctx.h, k, ptr, on_device)
        del keep
        return self

    def downsize(self, k: int) -> "ParamsKZG":
        """`ParamsKZG::downsize(k)` (kzg/commitment.rs:480-492), as a new object."""
        return ParamsKZG.__new__(ParamsKZG)._open_k(k, self.ctx, self.ctx.lib.cq_params_downsize, self.h, k)

    # ---- kzg/commitment.rs: read_custom, write_custom, g2, s_g2 ----
    @classmethod
    def _read(cls, ctx: Context, fn, data: bytes, flag: int) -> "ParamsKZG":
        buf = np.frombuffer(data, dtype=np.uint8)
        return cls.__new__(cls)._open_k(int.from_bytes(data[:4], "little"), ctx, fn, ctx.h, buf.ctypes.data, buf.shape[0], flag)

    @classmethod
    def read_raw(cls, ctx: Context, data: bytes, checked: bool = True) -> "ParamsKZG":
        """`ParamsKZG::read_custom(reader, RawBytes | RawBytesUnchecked)` (kzg/commitment.rs:383-459)."""
        return cls._read(ctx, ctx.lib.cq_params_read_raw, data, 1 if checked else 0)

    @classmethod
    def read(cls, ctx: Context, data: bytes, format: int = SERDE_PROCESSED) -> "ParamsKZG":
        """`ParamsKZG::read_custom(reader, format)` (kzg/commitment.rs:383-459); Processed points are decompressed on the GPU."""
        return cls._read(ctx, ctx.lib.cq_params_read, data, format)

    @classmethod
    def read_full(cls, ctx: Context, data: bytes, format: int = SERDE_PROCESSED) -> "ParamsKZG":
        """`ParamsKZG::read_custom(reader, format)` (kzg/commitment.rs:383-459), the complete stream: g2 and s_g2 are decompressed
        (Processed) or validated (RawBytes) on the GPU and kept."""
        return cls._read(ctx, ctx.lib.cq_params_read_full, data, format)

    def write_raw(self) -> bytes:
        """G1 part of `ParamsKZG::write_custom(writer, RawBytes)` (kzg/commitment.rs:366-379)."""
        return _written(4 + 128 * self.n, lambda buf, size, w: self.ctx._chk(self.ctx.lib.cq_params_write_raw(self.h, buf, size, w)))

    def write(self, format: int = SERDE_PROCESSED) -> bytes:
        """G1 part of `ParamsKZG::write_custom(writer, format)` (kzg/commitment.rs:366-379)."""
        lib = self.ctx.lib
        return _written(lib.cq_params_serialized_size(self.h, format),
                        lambda buf, size, w: self.ctx._chk(lib.cq_params_write(self.h, format, buf, size, w)))

    def write_full(self, format: int = SERDE_PROCESSED) -> bytes:
        """`ParamsKZG::write_custom(writer, format)` (kzg/commitment.rs:366-379), the complete stream; raises when no g2 / s_g2
        is held."""
        lib = self.ctx.lib
        return _written(lib.cq_params_serialized_size_full(self.h, format),
                        lambda buf, size, w: self.ctx._chk(lib.cq_params_write_full(self.h, format, buf, size, w)))

    def _tail(self):
        g2, s_g2 = np.zeros(16, dtype=np.uint64), np.zeros(16, dtype=np.uint64)
        self.ctx._chk(self.ctx.lib.cq_params_g2(self.h, g2.ctypes.data, s_g2.ctypes.data))
        return g2, s_g2

    # `ParamsKZG::g2()` / `s_g2()` (commitment.rs:351-358) as uint64[16]; CqError when the params hold none
    @property
    def g2(self):
        return self._tail()[0]

    @property
    def s_g2(self):
        return self._tail()[1]

    def set_g2(self, g2: np.ndarray, s_g2: np.ndarray):
        """stores `g2` and `s_g2` (uint64[16] each, raw layout) as given"""
        a = np.ascontiguousarray(g2, dtype=np.uint64).reshape(16)
        b = np.ascontiguousarray(s_g2, dtype=np.uint64).reshape(16)
        self.ctx._chk(self.ctx.lib.cq_params_set_g2(self.h, a.ctypes.data, b.ctypes.data))

    # ---- kzg/commitment.rs: get_g, commit, commit_lagrange ----
    @property
    def g_dev(self) -> int:
        return self.ctx.lib.cq_params_g_dev(self.h)

    @property
    def g_lagrange_dev(self) -> int:
        return self.ctx.lib.cq_params_g_lagrange_dev(self.h)

    def download(self):
        """(g, g_lagrange) as uint64[n,8] host arrays."""
        g = np.empty((self.n, 8), dtype=np.uint64)
        gl = np.empty((self.n, 8), dtype=np.uint64)
        self.ctx._chk(self.ctx.lib.cq_dev_download(self.ctx.h, g.ctypes.data, self.g_dev, g.nbytes))
        self.ctx._chk(self.ctx.lib.cq_dev_download(self.ctx.h, gl.ctypes.data, self.g_lagrange_dev, gl.nbytes))
        return g, gl

    def _commit(self, fn, poly):
        poly = _fr(poly)
        out = np.zeros(12, dtype=np.uint64)
        self.ctx._chk(fn(self.h, poly.ctypes.data, poly.shape[0], out.ctypes.data))
        return out

    def commit(self, poly: np.ndarray) -> np.ndarray:
        """`ParamsKZG::commit` (commitment.rs:539-543)."""
        return self._commit(self.ctx.lib.cq_commit, poly)

    def commit_lagrange(self, poly: np.ndarray) -> np.ndarray:
        """`ParamsKZG::commit_lagrange` (commitment.rs:496-504)."""
        return self._commit(self.ctx.lib.cq_commit_lagrange, poly)


class G2Srs(_Handle):
    """The G2 powers [s^i]_2 of `TableSRS` (poly/kzg/commitment.rs:73-123, field `g2`), resident on the GPU."""

    _destroy = "cq_g2_srs_destroy"

    # ---- kzg/commitment.rs (TableSRS) ----
    def __init__(self, ctx: Context, points: np.ndarray, checked: bool = True):
        p = _g2(points) if len(points) else np.zeros((0, 16), dtype=np.uint64)
        self.count = p.shape[0]
        self._open(ctx, ctx.lib.cq_g2_srs_create, ctx.h, self.count, p.ctypes.data, 1 if checked else 0)

    @classmethod
    def setup_from_toxic_waste(cls, ctx: Context, count: int, s: np.ndarray) -> "G2Srs":
        """[s^i]_2 for i < count, built on the GPU (the G2 half of TableSRS::setup_from_toxic_waste)."""
        self = cls.__new__(cls)
        self.count = count
        return self._open(ctx, ctx.lib.cq_g2_srs_setup_from_toxic_waste, ctx.h, count, _limbs4(s).ctypes.data)

    @classmethod
    def read(cls, ctx: Context, data: bytes, format: int = SERDE_PROCESSED) -> "G2Srs":
        """The G2 powers from the bytes `for p in srs.g2() { p.write(w, format) }` produces: points back to back, no header.
        Processed points are decompressed, RawBytes points validated, on the GPU; an invalid point is named by its index."""
        buf = np.frombuffer(data, dtype=np.uint8)
        self = cls.__new__(cls)._open(ctx, ctx.lib.cq_g2_srs_read, ctx.h, buf.ctypes.data if buf.shape[0] else None, buf.shape[0], format)
        self.count = ctx.lib.cq_g2_srs_len(self.h)
        return self

    def write(self, format: int = SERDE_PROCESSED) -> bytes:
        lib = self.ctx.lib
        return _written(lib.cq_g2_srs_serialized_size(self.h, format),
                        lambda buf, size, w: self.ctx._chk(lib.cq_g2_srs_write(self.h, format, buf, size, w)))

    @property
    def dev(self) -> int:
        return self.ctx.lib.cq_g2_srs_dev(self.h)

    def download(self) -> np.ndarray:
        p = np.empty((self.count, 16), dtype=np.uint64)
        self.ctx._chk(self.ctx.lib.cq_g2_srs_download(self.h, p.ctypes.data))
        return p


class TableConfig(_Handle):
    """`StaticTableConfig` (plonk/static_lookup.rs:47-66)."""

    _destroy = "cq_table_config_destroy"

    # ---- plonk/static_lookup.rs, kzg/commitment.rs (TableSRS) ----
    def __init__(self, ctx: Context, g1_lagrange: np.ndarray, g_lagrange_opening_at_0: np.ndarray):
        a, b = _g1(g1_lagrange), _g1(g_lagrange_opening_at_0)
        assert a.shape == b.shape
        self.size = a.shape[0]
        self._open(ctx, ctx.lib.cq_table_config_create, ctx.h, self.size, a.ctypes.data, b.ctypes.data)

    @classmethod
    def setup_from_toxic_waste(cls, ctx: Context, size: int, s: np.ndarray) -> "TableConfig":
        self = cls.__new__(cls)
        self.size = size
        return self._open(ctx, ctx.lib.cq_table_config_setup_from_toxic_waste, ctx.h, size, _limbs4(s).ctypes.data)

    @classmethod
    def from_srs(cls, ctx: Context, size: int, srs, srs_len: int | None = None) -> "TableConfig":
        """`StaticTableConfig` from the first `size` monomial powers [s^i]_1, no trapdoor: g1_lagrange = [L_i(s)]_1 and
        g_lagrange_opening_at_0 = [(L_i(s) - L_i(0)) / s]_1 (kzg/commitment.rs:125-170) as two inverse FFTs over G1.
        `srs`: a uint64[n,8] host array, a `ParamsKZG` (its resident g), or a device pointer (int / DevBuf) together with
        `srs_len`, the number of points behind it."""
        self = cls.__new__(cls)
        self.size = size
        if isinstance(srs, ParamsKZG):
            ptr, on_device, keep, srs_len = srs.g_dev, 1, srs, srs.n
        elif isinstance(srs, (int, np.integer, DevBuf)):
            if srs_len is None:
                raise CqError(-1, "TableConfig.from_srs: a device pointer needs srs_len")
            ptr, on_device, keep = _host_or_device_points(srs, 0)
        else:
            keep = _g1(srs)
            ptr, on_device = keep.ctypes.data, 0
            srs_len = keep.shape[0] if srs_len is None else min(srs_len, keep.shape[0])
        self._open(ctx, ctx.lib.cq_table_config_from_srs, ctx.h, size, ptr, srs_len, on_device)
        del keep
        return self

    def download(self):
        a = np.empty((self.size, 8), dtype=np.uint64)
        b = np.empty((self.size, 8), dtype=np.uint64)
        self.ctx._chk(self.ctx.lib.cq_table_config_download(self.h, a.ctypes.data, b.ctypes.data))
        return a, b


class StaticTable(_Handle):
    """`StaticTableValues` (plonk/static_lookup.rs:68-75)."""

    _destroy = "cq_static_table_destroy"

    def _open_values(self, values: np.ndarray, ctx: Context, create, *more) -> "StaticTable":
        """`create(ctx, size, values, *more, &handle)`"""
        v = _fr(values)
        self.size = v.shape[0]
        return self._open(ctx, create, ctx.h, self.size, v.ctypes.data, *more)

    # ---- plonk/static_lookup.rs ----
    def __init__(self, ctx: Context, values: np.ndarray, qs_affine: np.ndarray):
        v, q = _fr(values), _g1(qs_affine)
        assert v.shape[0] == q.shape[0]
        self._open_values(v, ctx, ctx.lib.cq_static_table_create, q.ctypes.data)

    @classmethod
    def setup_from_toxic_waste(cls, ctx: Context, values: np.ndarray, s: np.ndarray) -> "StaticTable":
        return cls.__new__(cls)._open_values(values, ctx, ctx.lib.cq_static_table_setup_from_toxic_waste, _limbs4(s).ctypes.data)

    @classmethod
    def new(cls, ctx: Context, values: np.ndarray, srs_g1: np.ndarray) -> "StaticTable":
        """`StaticTableValues::new(values, srs_g1)` (static_lookup.rs:78-126), the reference's O(N^2) construction."""
        v, g = _fr(values), _g1(srs_g1)
        assert v.shape[0] == g.shape[0]
        return cls.__new__(cls)._open_values(v, ctx, ctx.lib.cq_static_table_new, g.ctypes.data)

    @classmethod
    def new_fk(cls, ctx: Context, values: np.ndarray, srs_g1: np.ndarray | None = None, srs_dev=None) -> "StaticTable":
        """Same table as `StaticTable.new` (bit-identical cached quotients), built FK-style in O(N log N) group operations.
        The powers [s^i]_1 come from the host (`srs_g1`, uint64[N,8]) or are already resident (`srs_dev`: a device pointer or
        DevBuf to at least N affine points, e.g. `params.g_dev`)."""
        v = _fr(values)
        if (srs_g1 is None) == (srs_dev is None):
            raise CqError(-1, "StaticTable.new_fk: give srs_g1 or srs_dev")
        if srs_dev is not None:
            ptr = srs_dev.ptr if isinstance(srs_dev, DevBuf) else int(srs_dev)
            return cls.__new__(cls)._open_values(v, ctx, ctx.lib.cq_static_table_new_fk_dev, ptr)
        g = _g1(srs_g1)
        assert v.shape[0] == g.shape[0]
        return cls.__new__(cls)._open_values(v, ctx, ctx.lib.cq_static_table_new_fk, g.ctypes.data)

    def download_qs(self) -> np.ndarray:
        q = np.empty((self.size, 8), dtype=np.uint64)
        self.ctx._chk(self.ctx.lib.cq_static_table_download_qs(self.h, q.ctypes.data))
        return q

    def commit(self, srs_g2: "G2Srs", srs_g1_len: int, circuit_n: int):
        """`StaticTableValues::commit(srs_g2, srs_g1_len, circuit_n)` (static_lookup.rs:128-157): the verifying key's
        StaticCommittedTable as (zv, t, x_b0_bound), three affine G2 points (uint64[16] each)."""
        zv, t, xb = (np.zeros(16, dtype=np.uint64) for _ in range(3))
        self.ctx._chk(self.ctx.lib.cq_static_table_commit(self.h, srs_g2.h, srs_g1_len, circuit_n, zv.ctypes.data, t.ctypes.data,
                                                          xb.ctypes.data))
        return zv, t, xb


class EvaluationDomain(_Handle):
    """`EvaluationDomain<Fr>` (poly/domain.rs:19-34)."""

    _destroy = "cq_domain_destroy"

    # ---- poly/domain.rs ----
    def __init__(self, ctx: Context, j: int, k: int):
        self._open(ctx, ctx.lib.cq_domain_create, ctx.h, j, k)
        self.j = j
        self.k = k
        self.extended_k = ctx.lib.cq_domain_extended_k(self.h)
        self.n = 1 << k

    @property
    def extended_len(self) -> int:
        return 1 << self.extended_k

    def constants(self):
        arrs = [np.zeros(4, dtype=np.uint64) for _ in range(4)]
        self.ctx._chk(self.ctx.lib.cq_domain_constants(self.h, *[a.ctypes.data for a in arrs]))
        return dict(zip(("omega", "omega_inv", "extended_omega", "ifft_divisor"), arrs))

    def lagrange_to_coeff(self, a: np.ndarray) -> np.ndarray:
        a = _fr(a).copy()
        if a.shape[0] != self.n:  # domain.rs:239 assert
            raise CqError(-1, "lagrange_to_coeff: wrong length")
        self.ctx._chk(self.ctx.lib.cq_lagrange_to_coeff(self.h, a.ctypes.data))
        return a

    def coeff_to_extended(self, a: np.ndarray) -> np.ndarray:
        a = _fr(a)
        if a.shape[0] != self.n:  # domain.rs:256 assert
            raise CqError(-1, "coeff_to_extended: wrong length")
        out = np.zeros((self.extended_len, 4), dtype=np.uint64)
        self.ctx._chk(self.ctx.lib.cq_coeff_to_extended(self.h, a.ctypes.data, out.ctypes.data))
        return out

    def extended_to_coeff(self, a: np.ndarray) -> np.ndarray:
        a = _fr(a)
        if a.shape[0] != self.extended_len:  # domain.rs:294 assert
            raise CqError(-1, "extended_to_coeff: wrong length")
        out = np.zeros((self.n * (self.j - 1), 4), dtype=np.uint64)
        self.ctx._chk(self.ctx.lib.cq_extended_to_coeff(self.h, a.ctypes.data, out.ctypes.data))
        return out

    # device forms: `batch` columns stored back to back; they return once the work is queued on the context's stream
    def lagrange_to_coeff_dev(self, src: DevBuf, dst: DevBuf, batch: int = 1):
        """`batch` columns of n elements, stride n in and out; `dst` may be `src`."""
        self.ctx._chk(self.ctx.lib.cq_lagrange_to_coeff_dev(self.h, src.ptr, dst.ptr, batch))

    def coeff_to_extended_dev(self, src: DevBuf, dst: DevBuf, batch: int = 1):
        """`batch` columns of n coefficients (stride n) to columns of 2^extended_k evaluations; `dst` may not be `src`."""
        self.ctx._chk(self.ctx.lib.cq_coeff_to_extended_dev(self.h, src.ptr, dst.ptr, batch))

    def extended_to_coeff_dev(self, src: DevBuf, dst: DevBuf):
        """2^extended_k evaluations to n (j-1) coefficients, the only rows of `dst` written; `dst` may be `src`."""
        self.ctx._chk(self.ctx.lib.cq_extended_to_coeff_dev(self.h, src.ptr, dst.ptr))

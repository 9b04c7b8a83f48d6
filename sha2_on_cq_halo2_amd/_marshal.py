"""What every class of the binding needs to hand numpy arrays to the C ABI: array checks, ctypes helpers, the host-side
field helpers, and the structs, callback types and constants of include/cq_halo2.h (derived from the header by _lib.py)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import callback, constants, struct

# ---- include/cq_halo2.h: structs, callback types, constants --------------------------------------------
_CqPlonk, _CqCircuit, _BufferRng = struct("cq_plonk"), struct("cq_circuit"), struct("cq_buffer_rng")
_CqAssignedColumn, _CqXfer = struct("cq_assigned_column"), struct("cq_xfer")
_CqOpenQuery, _CqOpenTranscript = struct("cq_open_query"), struct("cq_open_transcript")

_SQUEEZE_T, _WRITE_POINT_T = callback("cq_squeeze_challenge_fn"), callback("cq_write_point_fn")
_ALLGATHER_T, _BCAST_T, _EXCHANGE_T = callback("cq_allgather_fn"), callback("cq_bcast_fn"), callback("cq_exchange_fn")
_PHASE_T = callback("cq_phase_fn")

_CQ = constants()
PROF_MSM_ACCUMULATE, PROF_NTT_PASS, PROF_MSM_ENTRIES, PROF_G1_DECOMPRESS, PROF_G2_DECOMPRESS = (
    _CQ["CQ_PROF_" + s] for s in ("MSM_ACCUMULATE", "NTT_PASS", "MSM_ENTRIES", "G1_DECOMPRESS", "G2_DECOMPRESS"))
# `SerdeFormat` (helpers.rs:8-20)
SERDE_PROCESSED, SERDE_RAW_BYTES, SERDE_RAW_BYTES_UNCHECKED = (_CQ["CQ_SERDE_" + s] for s in ("PROCESSED", "RAW_BYTES", "RAW_BYTES_UNCHECKED"))
FAIL_GATE, FAIL_GATE_POISONED, FAIL_LOOKUP, FAIL_STATIC_LOOKUP, FAIL_PERMUTATION = (
    _CQ["CQ_FAIL_" + s] for s in ("GATE", "GATE_POISONED", "LOOKUP", "STATIC_LOOKUP", "PERMUTATION"))
RCCL_UNIQUE_ID_BYTES = _CQ["CQ_RCCL_UNIQUE_ID_BYTES"]
_OPENERS = {"gwc": _CQ["CQ_OPENER_GWC"], "shplonk": _CQ["CQ_OPENER_SHPLONK"]}
SHA_ROT0, SHA_ROT1, SHA_MAJ, SHA_CH = 0, 1, 2, 3


# ---- array checks ---------------------------------------------------------------------------------------
def _limbs(a, width: int, what: str) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint64)
    assert a.ndim == 2 and a.shape[1] == width, f"expected uint64[n,{width}] {what}"
    return a


def _fr(a) -> np.ndarray:
    return _limbs(a, 4, "Montgomery limbs")


def _g1(a) -> np.ndarray:
    return _limbs(a, 8, "affine points")


def _g2(a) -> np.ndarray:
    return _limbs(a, 16, "G2 affine points")


def _fr_or_empty(a) -> np.ndarray:
    return _fr(a) if len(a) else np.zeros((0, 4), dtype=np.uint64)


def _limbs4(v) -> np.ndarray:
    return np.ascontiguousarray(v, dtype=np.uint64).reshape(4)


# ---- ctypes helpers -------------------------------------------------------------------------------------
def _ptr_array(ptrs, null_if_empty: bool):
    """void*[] of `ptrs`.  The C side tells an absent list (NULL) from an empty one in places, so every caller says which
    of the two no pointers stand for: None, or a (non-NULL) array."""
    ptrs = list(ptrs or [])
    return None if null_if_empty and not ptrs else (C.c_void_p * max(len(ptrs), 1))(*ptrs)


def _instance_columns(instances):
    """`instances: &[&[Fr]]` (prover.rs:64) as (column pointers, column lengths, keep-alive); NULLs for None."""
    if instances is None:
        return None, None, None
    cols = [_fr_or_empty(i) for i in instances]
    return _ptr_array([c.ctypes.data for c in cols], False), (C.c_size_t * max(len(cols), 1))(*[c.shape[0] for c in cols]), cols


class _ProofBuffer:
    """The (proof, capacity, &length) tail of the create_proof entry points."""

    def __init__(self, capacity: int):
        self.buf, self.len = (C.c_uint8 * capacity)(), C.c_size_t()
        self.args = (self.buf, capacity, C.byref(self.len))

    def bytes(self) -> bytes:
        return bytes(self.buf[: self.len.value])


def _written(size: int, write) -> bytes:
    """What `write(buffer, size, &written)` leaves in a buffer of `size` bytes."""
    buf = np.zeros(max(size, 1), dtype=np.uint8)
    w = C.c_size_t()
    write(buf.ctypes.data, size, C.byref(w))
    return buf[: w.value].tobytes()


def _struct_of(cls, *values):
    """`cls(*values)` where a pointer field may be given as an address (int or None)."""
    return cls(*[C.cast(v, t) if isinstance(v, (int, type(None))) and issubclass(t, C._Pointer) else v
                 for (_, t), v in zip(cls._fields_, values)])


def _assigned_structs(columns):
    """cq_assigned_column[] over the host arrays of plonk.AssignedColumn objects (which the caller keeps alive)."""
    arr = (_CqAssignedColumn * max(len(columns), 1))()
    for i, col in enumerate(columns):
        m = col.den_rows.shape[0]
        arr[i] = _struct_of(_CqAssignedColumn, col.num.ctypes.data, col.den_rows.ctypes.data if m else None,
                            col.den.ctypes.data if m else None, m)
    return arr


# ---- small host-side field helpers (Python ints; constants from bn256/fr.rs:29-83) ----------------
FR_MODULUS = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
FR_S = 28
FR_ROOT_OF_UNITY = 0x03DDB9F5166D18B798865EA93DD31F743215CF6DD39329C8D34F1ED960C37C9C


def fr_to_mont(v: int) -> np.ndarray:
    """canonical int -> uint64[4] Montgomery limbs (the layout every entry point takes)."""
    m = (v % FR_MODULUS) * (1 << 256) % FR_MODULUS
    return np.array([(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def fr_from_mont(limbs) -> int:
    m = sum(int(x) << (64 * i) for i, x in enumerate(np.asarray(limbs, dtype=np.uint64).reshape(4)))
    return m * pow(1 << 256, -1, FR_MODULUS) % FR_MODULUS


def domain_omega_int(k: int) -> int:
    """2^k-th root of unity as `EvaluationDomain::new` derives it (poly/domain.rs:54-75)."""
    w = FR_ROOT_OF_UNITY
    for _ in range(k, FR_S):
        w = w * w % FR_MODULUS
    return w


def domain_omega(k: int) -> np.ndarray:
    return fr_to_mont(domain_omega_int(k))

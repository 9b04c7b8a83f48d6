"""SerdeFormat::Processed without a GPU: the Fq square root of point decompression (csrc/sqrt29.hpp) built for the host and
run over its contract's edges, the new C ABI (header, exported symbols, Rust binding), and the test transcoder itself.
"""
import os
import random
import re
import subprocess

import numpy as np
import pytest

from oracle import bn254 as B
from oracle.cq_verifier import g1_from_bytes
from tests import field29_model as M
from tests import serde_processed_model as SM

ROOT = M.ROOT
Q = B.Q_MOD
RP = M.RP
REC_OUT = 29
SQRT_E = (Q + 1) // 4
NEW_FUNCTIONS = ["cq_g1_decompress_dev", "cq_g1_compress_dev", "cq_fr_from_repr_dev", "cq_fr_to_repr_dev", "cq_params_read",
                 "cq_params_write", "cq_params_serialized_size", "cq_pk_read", "cq_pk_write", "cq_pk_serialized_size"]
NEW_CONSTANTS = {"CQ_SERDE_PROCESSED": 0, "CQ_SERDE_RAW_BYTES": 1, "CQ_SERDE_RAW_BYTES_UNCHECKED": 2}


def _mont(v):
    return v * RP % Q


def _sqrt_inputs():
    """(label, operand limbs): the operand is a value's R' = 2^261 Montgomery form, unreduced where the contract allows"""
    rng = random.Random(29)
    out = [("a=%d" % a, M.norm(_mont(a))) for a in (0, 1, 4)] + [("a=q-1", M.norm(_mont(Q - 1)))]
    for i in range(200):  # squares of seeded uniform values
        out.append(("square#%d" % i, M.norm(_mont(pow(rng.randrange(Q), 2, Q)))))
    found = 0
    while found < 200:  # seeded non-residues, by Euler's criterion
        a = rng.randrange(1, Q)
        if pow(a, (Q - 1) // 2, Q) == Q - 1:
            out.append(("nonresidue#%d" % found, M.norm(_mont(a))))
            found += 1
    # the contract's edge: value < 8 q with limbs < 2^30 -- the largest values, normalised and with every lower limb as
    # large as allowed, the multiples of q around the representatives of 0, and uniform values with random spreading
    for form in M.forms(8, M.L30, Q, rng):
        out.append(("edge", form))
    for m in range(8):
        for d in (0, 1, -1):
            v = m * Q + d
            if 0 <= v < 8 * Q:
                out.append(("edge %dq%+d" % (m, d), M.norm(v)))
                out.append(("edge spread %dq%+d" % (m, d), M.spread(v, M.L30)))
    for i in range(200):
        out.append(("edge uniform#%d" % i, M.random_form(8, M.L30, Q, rng)))
    # what the decompression kernel hands over: x^3 R' + 3 R' as a limb-wise sum of two values below 2 q
    for i in range(100):
        u, v = rng.randrange(2 * Q), rng.randrange(2 * Q)
        out.append(("sum#%d" % i, [a + b for a, b in zip(M.norm(u), M.norm(v))]))
    return out


def test_sqrt29_host_build_matches_big_integers(tmp_path):
    """a^((q+1)/4) on 29-bit limbs, g++ build: the canonical result equals pow(a, (q+1)/4, q), `y^2 == a` is reported exactly
    when a is a square, and every intermediate value is normalised and below 2 q (the root check's difference: below 10 q) as the bound comments claim."""
    exe = os.path.join(str(tmp_path), "sqrt29_check")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", M.CSRC,
                        os.path.join(ROOT, "tests", "host", "sqrt29_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    inputs = _sqrt_inputs()
    for _, limbs in inputs:  # the operands respect the contract they are meant to probe
        assert M.val(limbs) < 8 * Q and all(x < M.L30 for x in limbs[:8])
    fin, fout = os.path.join(str(tmp_path), "in"), os.path.join(str(tmp_path), "out")
    np.array([l for _, l in inputs], dtype=np.uint32).tofile(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = np.fromfile(fout, dtype=np.uint32).reshape(len(inputs), REC_OUT)
    rinv = pow(RP, -1, Q)
    # intermediates the chain must show: 14 table entries, 4 squarings per digit below the top one, a product per non-zero
    # digit below the top one, and y^2 and the reduced difference of the root check
    digits = [(SQRT_E >> (4 * j)) & 15 for j in range(64)]
    top = max(j for j, d in enumerate(digits) if d)
    steps = 14 + 4 * top + sum(1 for d in digits[:top] if d) + 2
    bad = []
    for (label, limbs), o in zip(inputs, out):
        a = M.val(limbs) * rinv % Q
        want = pow(a, SQRT_E, Q)
        got = M.words_val(o[:8])
        if got != want:
            bad.append("%s: y = %x, want %x" % (label, got, want))
        is_square = want * want % Q == a
        if int(o[8]) != int(is_square):
            bad.append("%s: root check says %d, a is %sa square" % (label, o[8], "" if is_square else "not "))
        if int(o[9]) != 1:
            bad.append("%s: an intermediate value is not normalised" % label)
        if M.val(o[10:19]) >= 2 * Q:
            bad.append("%s: an intermediate value reaches %x >= 2 q" % (label, M.val(o[10:19])))
        diff = M.val(o[20:29])  # sub<8>(y^2, a) = y^2 + 8 q - a exactly, claimed < 10 q; Montgomery form
        if diff >= 10 * Q or (diff - (got * got - a) * RP) % Q:
            bad.append("%s: the root check's difference %x is not < 10 q or not y^2 - a" % (label, diff))
        if int(o[19]) != steps:
            bad.append("%s: %d intermediate values, expected %d" % (label, o[19], steps))
    assert not bad, bad[:10]
    # the labels mean what they say
    assert all(int(o[8]) == 1 for (l, _), o in zip(inputs, out) if l.startswith("square") or l in ("a=0", "a=1", "a=4"))
    assert all(int(o[8]) == 0 for (l, _), o in zip(inputs, out) if l.startswith("nonresidue") or l == "a=q-1")


def test_header_library_and_rust_binding_carry_the_processed_entry_points():
    from sha2_on_cq_halo2_amd import header_symbols, load

    header = open(os.path.join(ROOT, "include", "cq_halo2.h")).read()
    rs = open(os.path.join(ROOT, "include", "cq_halo2_sys.rs")).read()
    syms = header_symbols()
    lib = load()
    for fn in NEW_FUNCTIONS:
        assert fn in syms, fn
        assert hasattr(lib, fn), fn
        assert re.search(r"pub fn %s\(" % fn, rs), fn
    for name, value in NEW_CONSTANTS.items():
        m = re.search(r"^#define\s+%s\s+(\d+)" % name, header, flags=re.M)
        assert m and int(m.group(1)) == value, name
        assert re.search(r"pub const %s: i32 = %d;" % (name, value), rs), name  # one type for the enum, that of `format: c_int`
    from sha2_on_cq_halo2_amd import api

    assert (api.SERDE_PROCESSED, api.SERDE_RAW_BYTES, api.SERDE_RAW_BYTES_UNCHECKED) == (0, 1, 2)
    # host-only behaviour that needs no GPU: sizes of nothing, unknown formats
    assert lib.cq_params_serialized_size(None, 0) == 0 and lib.cq_pk_serialized_size(None, 0, 0) == 0


def test_transcoder_points_decode_to_the_points_it_started_from():
    from tests.util import random_points

    pts = random_points(40, 11)
    pts = pts + [B.g1_neg(p) for p in pts] + [None, B.G1_GEN, B.g1_neg(B.G1_GEN)]
    raw = B.points_to_mont_limbs(pts).tobytes()
    comp = SM.points_raw_to_processed(raw)
    assert len(comp) == 32 * len(pts)
    for i, p in enumerate(pts):
        b = comp[32 * i:32 * i + 32]
        assert g1_from_bytes(b) == p
        assert b == B.g1_to_bytes(p)
        assert SM.point_raw_to_affine(raw[64 * i:64 * i + 64]) == p
    # both sign bits occur for one x
    assert comp[:31] == comp[32 * 40:32 * 40 + 31] and comp[31] ^ comp[32 * 40 + 31] == 0x80
    # scalars, and a params stream
    vals = [0, 1, B.R_MOD - 1, 12345678901234567890]
    assert SM.scalars_raw_to_processed(B.to_mont_limbs(vals).tobytes()) == b"".join(v.to_bytes(32, "little") for v in vals)
    k = 3
    raw_params = (k).to_bytes(4, "little") + B.points_to_mont_limbs(pts[:8]).tobytes() + B.points_to_mont_limbs(pts[8:16]).tobytes()
    proc = SM.params_raw_to_processed(raw_params)
    assert len(proc) == 4 + 64 * 8 and proc[:4] == raw_params[:4]
    assert [g1_from_bytes(proc[4 + 32 * i:36 + 32 * i]) for i in range(16)] == pts[:16]


def test_transcoder_walks_the_proving_key_stream():
    """a synthetic raw key stream in the layout of oracle/serde.py: counts, lengths and selector bits pass through, the
    reported offsets point at the elements"""
    import struct

    from tests.util import random_points

    k, n, ext = 2, 4, 8
    pts = random_points(3, 5)  # 2 fixed + 1 permutation commitment
    rng = random.Random(3)
    polys = []

    def poly(ln):
        vals = [rng.randrange(B.R_MOD) for _ in range(ln)]
        polys.append(vals)
        return struct.pack(">I", ln) + B.to_mont_limbs(vals).tobytes()

    def slice_(cnt, ln):
        return struct.pack(">I", cnt) + b"".join(poly(ln) for _ in range(cnt))

    sel = bytes([0xA5])
    raw = struct.pack(">II", k, 2) + B.points_to_mont_limbs(pts).tobytes() + sel
    raw += poly(ext) + poly(ext) + poly(ext) + slice_(2, n) + slice_(2, n) + slice_(2, ext) + slice_(1, n) + slice_(1, n) + slice_(1, ext)
    layout = {}
    proc = SM.pk_raw_to_processed(raw, 1, 1, layout)
    assert len(proc) == len(raw) - 32 * 3
    assert proc[:8] == raw[:8] and proc[8 + 96:8 + 97] == sel
    assert [g1_from_bytes(proc[layout["commitments"] + 32 * i:layout["commitments"] + 32 * i + 32]) for i in range(3)] == pts
    assert len(layout["polys"]) == len(polys) == 12
    for (off, ln), vals in zip(layout["polys"], polys):
        assert ln == len(vals)
        assert [int.from_bytes(proc[off + 32 * i:off + 32 * i + 32], "little") for i in range(ln)] == vals
    with pytest.raises(AssertionError):
        SM.pk_raw_to_processed(raw + b"\0", 1, 1)

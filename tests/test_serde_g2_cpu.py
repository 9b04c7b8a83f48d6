"""G2 in the on-disk formats, without a GPU: the Fq2 square root of G2 point decompression (csrc/sqrt2_29.hpp) built for the
host and run over every class of operand against a literal restatement of the reference's Algorithm 9
(tests/serde_g2_model.py), the model's own round trips, and the new C ABI (header, exported symbols, Rust binding).
"""
import os
import random
import re
import subprocess

import numpy as np

from oracle import bn254 as B
from oracle import pairing as PR
from tests import field29_model as M
from tests import serde_g2_model as G

ROOT = M.ROOT
Q = B.Q_MOD
RP = M.RP
FQ2 = PR.FQ2
REC_OUT = 63
OPERAND_K = 8  # sqrt2_29.hpp: each component a value < 8 q with limbs < 2^30
NEW_FUNCTIONS = ["cq_g2_decompress_dev", "cq_g2_compress_dev", "cq_params_set_g2", "cq_params_g2", "cq_params_read_full",
                 "cq_params_write_full", "cq_params_serialized_size_full", "cq_g2_srs_read", "cq_g2_srs_write",
                 "cq_g2_srs_serialized_size"]


def _mont(v):
    return v * RP % Q


def _norm2(a):
    """an Fq2 element as two normalised limb lists of its R' Montgomery form"""
    return M.norm(_mont(a.c[0])), M.norm(_mont(a.c[1]))


def _legendre(v):
    return 0 if v % Q == 0 else (1 if pow(v, (Q - 1) // 2, Q) == 1 else -1)


def _sqrt2_inputs():
    """(label, c0 limbs, c1 limbs)"""
    rng = random.Random(2029)
    out = []

    def add(label, a):
        out.append((label,) + _norm2(a))

    for v in (0, 1, 4, Q - 1):
        add("real %s" % ("-1" if v == Q - 1 else v), FQ2([v, 0]))
    add("i", FQ2([0, 1]))
    add("-i", FQ2([0, Q - 1]))
    for i in range(200):  # squares of seeded general elements
        z = FQ2([rng.randrange(Q), rng.randrange(1, Q)])
        add("square#%d" % i, z * z)
    found = 0
    while found < 200:  # seeded non-squares, by the norm's Legendre symbol
        a = FQ2([rng.randrange(Q), rng.randrange(1, Q)])
        if _legendre(a.c[0] ** 2 + a.c[1] ** 2) == -1:
            add("nonsquare#%d" % found, a)
            found += 1
    res = non = 0
    while res < 100 or non < 100:  # real operands: a residue has the root (c, 0), a non-residue (0, c) -- the y.c0 == 0 case
        v = rng.randrange(1, Q)
        if _legendre(v) == 1 and res < 100:
            add("real residue#%d" % res, FQ2([v, 0]))
            res += 1
        elif _legendre(v) == -1 and non < 100:
            add("real nonresidue#%d" % non, FQ2([v, 0]))
            non += 1
    for i in range(100):
        add("imaginary#%d" % i, FQ2([0, rng.randrange(1, Q)]))
    # a.c0 + s == 0 with s = (a0^2 + a1^2)^((q+1)/4): forces a1 = 0 and a0 = -s for a residue s (the chain returns the residue
    # of the two roots) -- built from the chosen s
    for i in range(50):
        s = pow(rng.randrange(1, Q), 2, Q)
        assert pow(s * s % Q, (Q + 1) // 4, Q) == s
        add("a0 + s == 0 #%d" % i, FQ2([Q - s, 0]))
    # the contract's edges in each component (the other one uniform, and both at once)
    edge = M.forms(OPERAND_K, M.L30, Q, rng)
    for m in range(OPERAND_K):
        for d in (0, 1, -1):
            v = m * Q + d
            if 0 <= v < OPERAND_K * Q:
                edge += [M.norm(v), M.spread(v, M.L30)]
    for f in edge:
        out.append(("edge c0", f, M.random_form(OPERAND_K, M.L30, Q, rng)))
        out.append(("edge c1", M.random_form(OPERAND_K, M.L30, Q, rng), f))
        out.append(("edge c0, c1 = 0", f, M.norm(0)))
        out.append(("edge c1, c0 = 0", M.norm(0), f))
    for f in edge[:12]:
        for g in edge[:12]:
            out.append(("edge both", f, g))
    for i in range(200):
        out.append(("edge uniform#%d" % i, M.random_form(OPERAND_K, M.L30, Q, rng), M.random_form(OPERAND_K, M.L30, Q, rng)))
    # what the kernel hands over: x^3 + b' as a limb-wise sum of two values below 2 q per component
    for i in range(100):
        c = []
        for _ in range(2):
            u, v = rng.randrange(2 * Q), rng.randrange(2 * Q)
            c.append([a + b for a, b in zip(M.norm(u), M.norm(v))])
        out.append(("sum#%d" % i, c[0], c[1]))
    return out


def test_sqrt2_29_host_build_matches_algorithm_9(tmp_path):
    """the decoded y (both sign bits) and the is-a-square verdict of csrc/sqrt2_29.hpp, g++ build, against the model's
    Algorithm 9 + parity rule; every traced intermediate normalised and within the bound its comment claims"""
    exe = os.path.join(str(tmp_path), "sqrt2_29_check")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", M.CSRC,
                        os.path.join(ROOT, "tests", "host", "sqrt2_29_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    inputs = _sqrt2_inputs()
    for _, c0, c1 in inputs:  # the operands respect the contract they are meant to probe
        for limbs in (c0, c1):
            assert M.val(limbs) < OPERAND_K * Q and all(x < M.L30 for x in limbs[:8])
    fin, fout = os.path.join(str(tmp_path), "in"), os.path.join(str(tmp_path), "out")
    np.array([c0 + c1 for _, c0, c1 in inputs], dtype=np.uint32).tofile(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = np.fromfile(fout, dtype=np.uint32).reshape(len(inputs), REC_OUT)
    rinv = pow(RP, -1, Q)
    # values the tracer must see per run: a0, a1, n | chain 1 (14 table entries, 4 squarings per digit below the top one,
    # a product per non-zero digit below it) | s^2, its difference, the reduced difference | a0 - s, the two halves, a1 / 2 |
    # chain 2 | c, c^2, difference, reduced, a1 w / 2, its negation, reduced | canonical y.c0 and the two negations
    def chain(e):
        digits = [(e >> (4 * j)) & 15 for j in range(64)]
        top = max(j for j, d in enumerate(digits) if d)
        return 14 + 4 * top + sum(1 for d in digits[:top] if d)

    steps = 2 * (3 + chain((Q + 1) // 4) + 3 + 4 + chain((Q - 3) // 4) + 7 + 3)
    bad = []
    c0_zero = {"real nonresidue": 0, "a0 + s == 0": 0}
    for (label, l0, l1), o in zip(inputs, out):
        a = FQ2([M.val(l0) * rinv % Q, M.val(l1) * rinv % Q])
        root = G.fq2_sqrt(a)
        assert (root is not None) == G.fq2_is_square(a), label  # the model agrees with itself
        for key in c0_zero:
            if label.startswith(key):  # the ambiguous case is really exercised: Algorithm 9's root has c0 == 0 there
                assert root is not None and root.c[0] == 0 and root.c[1] != 0, label
                c0_zero[key] += 1
        for ysign in (0, 1):
            rec = o[17 * ysign:17 * ysign + 17]
            want = G.apply_sign(root, ysign)  # = G.decoded_y(a, ysign), with the root computed once
            if int(rec[16]) != int(want is not None):
                bad.append("%s sign %d: verdict %d, a is %sa square" % (label, ysign, rec[16], "" if want is not None else "not "))
            if want is not None:
                got = FQ2([M.words_val(rec[:8]), M.words_val(rec[8:16])])
                if got != want:
                    bad.append("%s sign %d: y = %s, want %s" % (label, ysign, [hex(v) for v in got.c], [hex(v) for v in want.c]))
        if int(o[34]) != 1:
            bad.append("%s: an intermediate value is not normalised" % label)
        if int(o[35]) != steps:
            bad.append("%s: %d intermediate values, expected %d" % (label, o[35], steps))
        if M.val(o[36:45]) >= 2 * Q:
            bad.append("%s: a value claimed < 2 q reaches %x" % (label, M.val(o[36:45])))
        if M.val(o[45:54]) >= 4 * Q:
            bad.append("%s: a value claimed < 4 q reaches %x" % (label, M.val(o[45:54])))
        if M.val(o[54:63]) > 2 * Q:
            bad.append("%s: a negation claimed <= 2 q reaches %x" % (label, M.val(o[54:63])))
    assert not bad, bad[:10]
    assert c0_zero == {"real nonresidue": 100, "a0 + s == 0": 50}
    # the labels mean what they say
    for (label, _, _), o in zip(inputs, out):
        if label.startswith(("square", "real", "imaginary", "a0 + s")) or label in ("i", "-i"):
            assert int(o[16]) == 1 and int(o[33]) == 1, label  # every element of Fq is a square in Fq2; so is +-i times one
        if label.startswith("nonsquare"):
            assert int(o[16]) == 0 and int(o[33]) == 0, label


def _model_points():
    rng = B.Xoshiro256ss(0x62D0)
    pos = [PR.g2_mul(B.fr_random(rng)) for _ in range(40)]
    return pos + [PR.ec_neg(p) for p in pos] + [None, PR.G2_GEN]


def test_model_round_trips_and_byte_layout():
    pts = _model_points()
    signs = set()
    for p in pts:
        b = G.g2_to_bytes(p)
        assert len(b) == 64 and G.g2_from_bytes(b) == p
        if p is None:
            assert b == bytes(64)
            continue
        assert PR.is_on_twist(p)
        signs.add(b[63] >> 7)
        # c0 then c1, canonical little-endian; the sign bit is bit 7 of byte 63 and the parity of the canonical y.c0
        assert int.from_bytes(b[:32], "little") == p[0].c[0]
        assert int.from_bytes(b[32:], "little") & ((1 << 255) - 1) == p[0].c[1]
        assert b[63] >> 7 == p[1].c[0] & 1
        # through the raw layout and the transcoder
        raw = G.point_affine_to_raw(p)
        assert G.point_raw_to_affine(raw) == p and G.points_raw_to_processed(raw) == b
    assert signs == {0, 1}
    # P and -P share the x bytes and differ in the sign bit alone
    b0, b1 = G.g2_to_bytes(pts[0]), G.g2_to_bytes(pts[40])
    assert b0[:63] == b1[:63] and b0[63] ^ b1[63] == 0x80
    # b' is not a square: x = 0 is on no point, with either sign bit... and with the bit clear it is the identity
    assert not G.fq2_is_square(PR.B2)
    bad = bytearray(64)
    bad[63] = 0x80
    try:
        G.g2_from_bytes(bytes(bad))
        raise AssertionError("x = 0 with the sign bit decoded")
    except ValueError:
        pass
    # the full params stream: the G1 part by the G1 transcoder, then the two tail points
    from tests.util import random_points

    k = 2
    g1 = B.points_to_mont_limbs(random_points(8, 3)).tobytes()
    raw = (k).to_bytes(4, "little") + g1 + G.point_affine_to_raw(PR.G2_GEN) + G.point_affine_to_raw(pts[3])
    proc = G.params_full_raw_to_processed(raw)
    assert len(proc) == 4 + 64 * 4 + 128
    assert G.g2_from_bytes(proc[-128:-64]) == PR.G2_GEN and G.g2_from_bytes(proc[-64:]) == pts[3]


def test_header_library_and_rust_binding_carry_the_g2_entry_points():
    from sha2_on_cq_halo2_amd import header_symbols, load

    rs = open(os.path.join(ROOT, "include", "cq_halo2_sys.rs")).read()
    syms = header_symbols()
    lib = load()
    for fn in NEW_FUNCTIONS:
        assert fn in syms, fn
        assert hasattr(lib, fn), fn
        assert re.search(r"pub fn %s\(" % fn, rs), fn
    # host-only behaviour that needs no GPU: sizes of nothing, unknown formats
    for fmt in (0, 1, 2, 7):
        assert lib.cq_params_serialized_size_full(None, fmt) == 0
        assert lib.cq_g2_srs_serialized_size(None, fmt) == 0

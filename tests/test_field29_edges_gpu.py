"""The lazy 29-bit field arithmetic and the XYZZ group laws on it, built for gfx950 and run on the GPU, at the edges of their
bound contracts.

* The records of tests/test_field29_edges_cpu.py (contract edges, maximal columns, uniform operands, every annotated call
  site at its extreme) through the gfx950 build of tests/host/field29_edges.cpp: byte-equal to the host build's output,
  and exact / within bounds by tests/field29_model.py.
* G1 xyzz29_add / _add_affine / _dbl / _dbl_affine / quad_add and G2 xyzz2_add / _add_affine / _dbl / _dbl_affine
  (tests/host/curve29_edges.hip) on coordinates at the top of the headers' invariants (G1: x + 7 p, y + 3 p, zz + p,
  zzz + p; G2: every component + p), after a store / load round trip, on equal points in different scalings (doubling
  reached through is_zero_mod_p of a non-zero multiple of p), P + (-P) in different scalings, and identities; compared with
  oracle/bn254.py and oracle/pairing.py as affine points.
"""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from oracle import bn254 as B
from oracle import pairing as PR
from tests import field29_model as M
from tests.test_field29_edges_cpu import SITES

pytestmark = pytest.mark.gpu

Q = B.Q_MOD
RP = M.RP


def test_field29_edges_gfx950_byte_equal_to_host(tmp_path):
    """Every record of the CPU test through the gfx950 build: the same bytes as the host build, and exact / in bounds."""
    recs = M.build_records(seed=1, per_op=2000, table=SITES)
    host = M.run(M.build_host(tmp_path), recs, tmp_path, "host")
    dev = M.run(M.build_device(tmp_path), recs, tmp_path, "dev", timeout=120)
    diff = np.nonzero((dev != host).any(axis=1))[0]
    assert diff.size == 0, ["%s %s %s" % (recs[i].src, recs[i].field, recs[i].op) for i in diff[:20]]
    bad = M.check(recs, dev)
    assert not bad, "\n".join(bad[:40])


# ---- group law -----------------------------------------------------------------------------------------------------------
G1_ADD, G1_ADD_AFFINE, G1_DBL, G1_DBL_AFFINE, G1_QUAD_ADD, G1_ADD_STORED = range(6)
G2_ADD, G2_ADD_AFFINE, G2_DBL, G2_DBL_AFFINE, G2_ADD_STORED = range(6, 11)


def _r(v, k):
    """the R' limb form of field element v, plus k p (normalised limbs)"""
    return M.norm(v * RP % Q + k * Q)


def _fq2(c, k):
    return _r(c.c[0], k) + _r(c.c[1], k)


def g1_xyzz(P, lam, top):
    """P in XYZZ with scaling lam, coordinates raised to the top of the invariant (x < 8 p, y < 4 p, zz, zzz < 2 p)"""
    if P is None:
        return [0] * 36
    l2, l3 = lam * lam % Q, lam * lam * lam % Q
    ks = (7, 3, 1, 1) if top else (0, 0, 0, 0)
    return _r(P[0] * l2, ks[0]) + _r(P[1] * l3, ks[1]) + _r(l2, ks[2]) + _r(l3, ks[3])


def g1_aff(P, top):
    return [0] * 18 if P is None else _r(P[0], int(top)) + _r(P[1], int(top))


def g2_xyzz(P, lam, top):
    if P is None:
        return [0] * 72
    k = int(top)
    l2 = lam * lam
    l3 = l2 * lam
    return _fq2(P[0] * l2, k) + _fq2(P[1] * l3, k) + _fq2(l2, k) + _fq2(l3, k)


def g2_aff(P, top):
    return [0] * 36 if P is None else _fq2(P[0], int(top)) + _fq2(P[1], int(top))


def _val(limbs):
    return M.val(limbs)


def decode_g1(o):
    """(affine point or None, invariant ok)"""
    c = [o[9 * k:9 * k + 9] for k in range(4)]
    ok = all(x <= M.M29 for l in c for x in l[:8]) and _val(c[0]) < 8 * Q and _val(c[1]) < 4 * Q and _val(c[2]) < 2 * Q \
        and _val(c[3]) < 2 * Q
    if not any(c[2]):
        return None, ok
    x, y, zz, zzz = (_val(l) for l in c)
    # (the R' factors cancel in the ratios; zz^3 = zzz^2 up to them: zz^3 / R'^3 = zzz^2 / R'^2)
    ok = ok and (zz ** 3 - zzz ** 2 * RP) % Q == 0
    return (x * pow(zz, -1, Q) % Q, y * pow(zzz, -1, Q) % Q), ok


def decode_g2(o):
    comps = [_val(o[9 * k:9 * k + 9]) for k in range(8)]
    ok = all(x <= M.M29 for k in range(8) for x in o[9 * k:9 * k + 8]) and all(v < 2 * Q for v in comps)
    if not any(o[36:54]):
        return None, ok
    rinv = pow(RP, -1, Q)
    f = [PR.FQ2([comps[2 * k] * rinv % Q, comps[2 * k + 1] * rinv % Q]) for k in range(4)]
    return (f[0] / f[2], f[1] / f[3]), ok


def g1_records(rng):
    recs = []  # (op, A limbs, B limbs, expected affine point)
    pts = [B.g1_mul(B.G1_GEN, k) for k in (1, 2, 3, 5, 7, 123456789, B.R_MOD - 1)] + [B.g1_mul(B.G1_GEN, rng.randrange(B.R_MOD)) for _ in range(3)]
    lam = lambda: rng.randrange(2, Q)  # noqa: E731
    for i, P in enumerate(pts):
        Qp = pts[(i + 1) % len(pts)]
        negP = B.g1_neg(P)
        for top in (True, False):
            for op in (G1_ADD, G1_QUAD_ADD, G1_ADD_STORED):
                recs.append((op, g1_xyzz(P, lam(), top), g1_xyzz(Qp, lam(), top), B.g1_add(P, Qp)))
                recs.append((op, g1_xyzz(P, lam(), top), g1_xyzz(P, lam(), not top), B.g1_add(P, P)))   # doubling, other scaling
                recs.append((op, g1_xyzz(P, 1, top), g1_xyzz(P, 1, top), B.g1_add(P, P)))               # bit-identical
                recs.append((op, g1_xyzz(P, lam(), top), g1_xyzz(negP, lam(), top), None))              # cancellation
                recs.append((op, g1_xyzz(P, lam(), top), g1_xyzz(None, 1, top), P))
                recs.append((op, g1_xyzz(None, 1, top), g1_xyzz(P, lam(), top), P))
            recs.append((G1_ADD_AFFINE, g1_xyzz(P, lam(), top), g1_aff(Qp, top), B.g1_add(P, Qp)))
            recs.append((G1_ADD_AFFINE, g1_xyzz(P, lam(), top), g1_aff(P, not top), B.g1_add(P, P)))
            recs.append((G1_ADD_AFFINE, g1_xyzz(P, lam(), top), g1_aff(negP, top), None))
            recs.append((G1_ADD_AFFINE, g1_xyzz(None, 1, top), g1_aff(P, top), P))
            recs.append((G1_ADD_AFFINE, g1_xyzz(P, lam(), top), g1_aff(None, top), P))
            recs.append((G1_DBL, g1_xyzz(P, lam(), top), [], B.g1_add(P, P)))
            recs.append((G1_DBL_AFFINE, g1_aff(P, top), [], B.g1_add(P, P)))
        recs.append((G1_ADD, [0] * 36, [0] * 36, None))
        recs.append((G1_QUAD_ADD, [0] * 36, [0] * 36, None))
        recs.append((G1_DBL, [0] * 36, [], None))
        recs.append((G1_DBL_AFFINE, [0] * 18, [], None))
    return recs


def g2_records(rng):
    recs = []
    pts = [PR.G2_GEN]
    for _ in range(4):
        pts.append(PR.ec_add(pts[-1], PR.G2_GEN))
    pts.append(PR.g2_mul(rng.randrange(B.R_MOD)))
    lam = lambda: PR.FQ2([rng.randrange(1, Q), rng.randrange(Q)])  # noqa: E731
    one = PR.FQ2([1, 0])
    for i, P in enumerate(pts):
        Qp = pts[(i + 1) % len(pts)]
        negP = PR.ec_neg(P)
        two = PR.ec_double(P)
        for top in (True, False):
            for op in (G2_ADD, G2_ADD_STORED):
                recs.append((op, g2_xyzz(P, lam(), top), g2_xyzz(Qp, lam(), top), PR.ec_add(P, Qp)))
                recs.append((op, g2_xyzz(P, lam(), top), g2_xyzz(P, lam(), not top), two))
                recs.append((op, g2_xyzz(P, one, top), g2_xyzz(P, one, top), two))
                recs.append((op, g2_xyzz(P, lam(), top), g2_xyzz(negP, lam(), top), None))
                recs.append((op, g2_xyzz(P, lam(), top), g2_xyzz(None, one, top), P))
                recs.append((op, g2_xyzz(None, one, top), g2_xyzz(P, lam(), top), P))
            recs.append((G2_ADD_AFFINE, g2_xyzz(P, lam(), top), g2_aff(Qp, top), PR.ec_add(P, Qp)))
            recs.append((G2_ADD_AFFINE, g2_xyzz(P, lam(), top), g2_aff(P, not top), two))
            recs.append((G2_ADD_AFFINE, g2_xyzz(P, lam(), top), g2_aff(negP, top), None))
            recs.append((G2_ADD_AFFINE, g2_xyzz(None, one, top), g2_aff(P, top), P))
            recs.append((G2_ADD_AFFINE, g2_xyzz(P, lam(), top), g2_aff(None, top), P))
            recs.append((G2_DBL, g2_xyzz(P, lam(), top), [], two))
            recs.append((G2_DBL_AFFINE, g2_aff(P, top), [], two))
    recs.append((G2_DBL, [0] * 72, [], None))
    recs.append((G2_DBL_AFFINE, [0] * 36, [], None))
    return recs


def test_group_law_with_extreme_representatives(tmp_path):
    """Every G1 / G2 XYZZ formula on extreme representatives gives the oracle's affine point and keeps the invariant."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    root = M.ROOT
    exe = str(tmp_path / "curve29_edges")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(root, "include"), "-I", M.CSRC,
                        os.path.join(root, "tests", "host", "curve29_edges.hip"), "-o", exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    rng = random.Random(29)
    recs = g1_records(rng) + g2_records(rng)
    a = np.zeros((len(recs), 1 + 144), dtype=np.uint32)
    for i, (op, A, Bl, _) in enumerate(recs):
        a[i, 0] = op
        a[i, 1:1 + len(A)] = A
        a[i, 73:73 + len(Bl)] = Bl
    fin, fout = str(tmp_path / "g.in"), str(tmp_path / "g.out")
    a.tofile(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-1000:])
    out = np.fromfile(fout, dtype=np.uint32).reshape(len(recs), 72)
    bad = []
    for i, (op, A, Bl, want) in enumerate(recs):
        o = [int(x) for x in out[i]]
        got, ok = decode_g1(o) if op < G2_ADD else decode_g2(o)
        if not ok:
            bad.append("record %d op %d: result outside the invariant" % (i, op))
        if got != want:
            bad.append("record %d op %d: wrong point" % (i, op))
    assert not bad, "\n".join(bad[:40]) + "\n(%d records)" % len(recs)

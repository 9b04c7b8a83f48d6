"""Big-integer model and edge vectors of the lazy 29-bit field arithmetic (csrc/field29.hpp Fp29, csrc/field2_29.hpp Fq2_29).

The values of that arithmetic are not reduced: a value may range over [0, K p) and limbs may be unnormalised, and every
operation states how far (field29.hpp, field2_29.hpp; the call sites annotate the bounds they rely on).  This module builds
operands on the edges of those contracts -- K p - 1 normalised and with every lower limb as large as allowed, 0, p, the
Ka Kb = 128 pairs, maximal six-product columns, every annotated call site at its extreme -- plus seeded uniform ones, runs
them through tests/host/field29_edges.cpp (a host build, or the gfx950 build) and checks each output:
  * the exact result: REDC(T) = (T + (T (-p^-1) mod 2^261) p) / 2^261 as normalised limbs for the products, the exact
    integer a + K p - b for sub / neg (so a carry lost in a 64-bit column or a limb that wrapped shows up bit for bit);
  * the value mod p, computed from the field formula alone (x y 2^-261, the Fq2 product, ...);
  * the stated postcondition: limbs 0..7 < 2^29, value below the bound the contract or the call site claims.
"""
import itertools
import os
import random
import subprocess

import numpy as np

from oracle import bn254 as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sha2_on_cq_halo2_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "host", "field29_edges.cpp")

M29 = (1 << 29) - 1
L29, L30, L31 = 1 << 29, 1 << 30, 1 << 31
L3 = 3 << 29  # limbs of the PAD-31 subtrahend ppp + q + q
RP = 1 << 261  # R' of the limb form
W = "w"  # operand bound: a memory word read as limbs (value < 2^256)
NOPS, REC_IN, REC_OUT = 12, 109, 32
FIELDS = {"q": (0, B.Q_MOD), "r": (1, B.R_MOD)}

# name -> (code, operands, Fp29 outputs); codes as in field29_edges.cpp
OPS = {
    "mul": (0, 2, 1), "mul2": (1, 4, 1),
    "mac1": (2, 2, 1), "mac2": (3, 4, 1), "mac3": (4, 6, 1), "mac4": (5, 8, 1), "mac5": (6, 10, 1), "mac6": (7, 12, 1),
    "sqr": (8, 1, 1), "mul_pair": (9, 4, 2), "sqr_pair": (10, 2, 2), "mul2_mul_mul": (11, 8, 3),
    "sub2": (12, 2, 1), "sub4": (13, 2, 1), "sub8": (14, 2, 1), "sub16": (15, 2, 1), "sub32": (16, 2, 1), "sub64": (17, 2, 1),
    "sub6_31": (18, 2, 1), "neg2": (19, 1, 1), "neg4": (20, 1, 1),
    "normalise": (21, 1, 1), "reduced": (22, 1, 1), "is_zero": (23, 1, 0), "canon": (24, 1, 0), "to_mont256": (25, 1, 0),
    "from_mont256": (26, 1, 1), "pack": (27, 1, 0), "unpack": (28, 1, 1),
    "mul_pair_alias": (29, 4, 2), "mul_pair_alias2": (30, 4, 2),
    # Fq2_29 (Fq only): operands are (c0, c1) pairs
    "f2mul2": (64, 4, 2), "f2mul6": (65, 4, 2), "f2sqr2": (66, 2, 2), "f2sqr4": (67, 2, 2), "f2mul2_42": (68, 8, 2),
}
SUB_K = {"sub2": 2, "sub4": 4, "sub8": 8, "sub16": 16, "sub32": 32, "sub64": 64, "sub6_31": 6}


# ---- limb forms ---------------------------------------------------------------------------------------------------------
def val(limbs):
    return sum(int(x) << (29 * i) for i, x in enumerate(limbs))


def norm(v):
    """normalised limbs (0..7 < 2^29, the top limb the rest)"""
    assert 0 <= v and v >> 232 < (1 << 32), hex(v)
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def spread(v, lim, rng=None):
    """v with every lower limb as large as possible below lim (or a random amount of spreading with rng)"""
    out = []
    for _ in range(8):
        r = v & M29
        k = min((lim - 1 - r) >> 29, v >> 29)
        if rng is not None and k > 0:
            k = rng.randint(0, k)
        out.append(r + (k << 29))
        v = (v - out[-1]) >> 29
    assert v < (1 << 32)
    return out + [v]


def words(v):
    assert 0 <= v < (1 << 256)
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def words_val(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w[:8]))


_NINV = {}


def redc(T, p):
    if p not in _NINV:
        _NINV[p] = (-pow(p, -1, RP)) % RP
    return (T + (T * _NINV[p] % RP) * p) >> 261


# ---- records ----------------------------------------------------------------------------------------------------------
class Rec:
    """one driver record: field, operation, operand limb lists, the bound claimed for the result (multiple of p, None:
    exactness only), and where it comes from"""
    __slots__ = ("field", "op", "ops", "claim", "src")

    def __init__(self, field, op, ops, claim, src):
        self.field, self.op, self.ops, self.claim, self.src = field, op, ops, claim, src


def encode(recs):
    a = np.zeros((len(recs), REC_IN), dtype=np.uint32)
    for i, r in enumerate(recs):
        fid = FIELDS[r.field][0]
        a[i, 0] = (fid << 8) | OPS[r.op][0]
        for k, l in enumerate(r.ops):
            a[i, 1 + 9 * k:10 + 9 * k] = l
    return a


def expected(r):
    """(exact output u32 list, list of output values to hold to the postcondition, value check ok)"""
    p = FIELDS[r.field][1]
    v = [val(l) for l in r.ops]
    op = r.op
    rinv = pow(RP, -1, p)
    prods = None  # the products each output holds, for the independent mod-p check
    if op == "mul":
        prods = [v[0] * v[1]]
    elif op == "mul2":
        prods = [v[0] * v[1] + v[2] * v[3]]
    elif op.startswith("mac"):
        n = int(op[3:])
        prods = [sum(v[2 * k] * v[2 * k + 1] for k in range(n))]
    elif op == "sqr":
        prods = [v[0] * v[0]]
    elif op in ("mul_pair", "mul_pair_alias"):
        prods = [v[0] * v[1], v[2] * v[3]]
    elif op == "mul_pair_alias2":
        prods = [v[0] * v[1], v[1] * v[3]]
    elif op == "sqr_pair":
        prods = [v[0] * v[0], v[1] * v[1]]
    elif op == "mul2_mul_mul":
        prods = [v[0] * v[1] + v[2] * v[3], v[4] * v[5], v[6] * v[7]]
    if prods is not None:
        outs = [redc(t, p) for t in prods]
        ok = all((o - t * rinv) % p == 0 for o, t in zip(outs, prods))
        return sum((norm(o) for o in outs), []), outs, ok
    if op in SUB_K:
        o = v[0] + SUB_K[op] * p - v[1]
        return norm(o), [o], True
    if op in ("neg2", "neg4"):
        o = int(op[3:]) * p - v[0]
        return norm(o), [o], True
    if op == "normalise":
        return norm(v[0]), [v[0]], True
    if op == "reduced":
        o = redc(v[0] * (RP % p), p)
        return norm(o), [o], (o - v[0]) % p == 0
    if op == "is_zero":
        return [int(v[0] % p == 0), int(v[0] == 0)], [], True
    if op in ("canon", "to_mont256"):
        c = RP % p if op == "canon" else (1 << 256) % p
        o = redc(v[0] * c, p)
        o = o - p if o >= p else o
        want = v[0] % p if op == "canon" else v[0] * (1 << 256) * rinv % p
        return words(o), [o], o == want
    if op == "from_mont256":
        y = words_val(r.ops[0])
        o = redc(y * ((1 << 266) % p), p)
        return norm(o), [o], (o - y * 32) % p == 0
    if op == "pack":
        return words(v[0]), [], True
    if op == "unpack":
        y = words_val(r.ops[0])
        return norm(y), [y], True
    if op.startswith("f2"):
        if op in ("f2mul2", "f2mul6", "f2mul2_42"):
            # a = (v0, v1), b = (v2, v3) [, c = (v4, v5), d = (v6, v7)]; the negated b1 / d1 as the header forms them
            kb = {"f2mul2": 2, "f2mul6": 6, "f2mul2_42": 4}[op]
            t0 = v[0] * v[2] + v[1] * (kb * p - v[3])
            t1 = v[0] * v[3] + v[1] * v[2]
            want = ((v[0] * v[2] - v[1] * v[3]), (v[0] * v[3] + v[1] * v[2]))
            if op == "f2mul2_42":
                t0 += v[4] * v[6] + v[5] * (2 * p - v[7])
                t1 += v[4] * v[7] + v[5] * v[6]
                want = (want[0] + v[4] * v[6] - v[5] * v[7], want[1] + v[4] * v[7] + v[5] * v[6])
        else:
            ka = 2 if op == "f2sqr2" else 4
            t0 = (v[0] + v[1]) * (v[0] + ka * p - v[1])
            t1 = 2 * v[0] * v[1]
            want = (v[0] * v[0] - v[1] * v[1], 2 * v[0] * v[1])
        outs = [redc(t0, p), redc(t1, p)]
        ok = all((o - w * rinv) % p == 0 for o, w in zip(outs, want))
        return norm(outs[0]) + norm(outs[1]), outs, ok
    raise ValueError(op)


def check(recs, out):
    """every disagreement as a readable line (empty: all records good)"""
    bad = []
    for i, r in enumerate(recs):
        exp, outs, ok = expected(r)
        got = [int(x) for x in out[i, :len(exp)]]
        where = "%s %s %s" % (r.src, r.field, r.op)
        if got != exp:
            bad.append("%s: output %s != exact %s (operands %s)" % (where, got, exp, [hex(val(l)) for l in r.ops]))
            continue
        if not ok:
            bad.append("%s: wrong value mod p" % where)
        p = FIELDS[r.field][1]
        nlimbs = OPS[r.op][2]
        for k in range(nlimbs):
            if any(x > M29 for x in got[9 * k:9 * k + 8]):
                bad.append("%s: output %d not normalised" % (where, k))
        if r.claim is not None:
            for o in outs:
                # (neg<K> returns K p itself for 0: its bound is <= K p)
                if o > r.claim * p or (o == r.claim * p and r.op not in ("neg2", "neg4")):
                    bad.append("%s: result %s >= %s p (claimed)" % (where, hex(o), r.claim))
        if len(bad) > 40:
            break
    return bad


# ---- operand generation ------------------------------------------------------------------------------------------------
def bound(k, p):
    return (1 << 256) if k == W else k * p


def forms(k, lim, p, rng):
    """the edge representatives of an operand < k p with limbs < lim: k p - 1 normalised and spread, 0, 1, p - 1, p,
    p + 1, 2 p - 1 where below the bound, and one uniform value with random spreading"""
    b = bound(k, p)
    vals = [b - 1, 0, 1, p - 1, p, p + 1, 2 * p - 1]
    out = [norm(b - 1), spread(b - 1, lim)] if lim > L29 else [norm(b - 1)]
    for v in vals[1:]:
        if v < b:
            out.append(norm(v))
    out.append(spread(rng.randrange(b), lim, rng))
    if lim > L29:  # every lower limb at lim - 1 and the top limb as large as the bound allows
        low = sum((lim - 1) << (29 * i) for i in range(8))
        if low < b:
            out.append([lim - 1] * 8 + [(b - 1 - low) >> 232])
    return out


def random_form(k, lim, p, rng):
    return spread(rng.randrange(bound(k, p)), lim, rng)


def case_records(field, op, specs, claim, src, rng, combos=64):
    """the extreme combinations of the operands' edge forms (all of them for up to two operands, `combos` random picks of
    them beyond that, always including every operand at its maximum in both forms)"""
    p = FIELDS[field][1]
    fs = [forms(k, lim, p, rng) for k, lim in specs]
    recs = []
    if len(fs) <= 2:
        for c in itertools.product(*fs):
            recs.append(Rec(field, op, [list(x) for x in c], claim, src))
    else:
        recs.append(Rec(field, op, [f[0] for f in fs], claim, src))
        recs.append(Rec(field, op, [f[1] if len(f) > 1 else f[0] for f in fs], claim, src))
        for _ in range(combos):
            recs.append(Rec(field, op, [rng.choice(f) for f in fs], claim, src))
    return recs


def random_records(field, op, specs, claim, src, rng, n):
    p = FIELDS[field][1]
    return [Rec(field, op, [random_form(k, lim, p, rng) for k, lim in specs], claim, src) for _ in range(n)]


# The contracts of the headers, at their edges: op -> list of (operand specs (K, limb limit), claimed result bound)
def _pairs128(lim):
    return [((ka, lim), (128 // ka, lim)) for ka in (1, 2, 4, 8, 16, 32, 64, 128)]


def contracts():
    c = {}
    c["mul"] = [(list(s), 2) for s in _pairs128(L30)]                                   # Ka Kb <= 128, limbs < 2^30
    c["sqr"] = [([(11, L30)], 2)]                                                       # 121
    c["mul_pair"] = [([(64, L30), (2, L30), (2, L30), (64, L30)], 2), ([(11, L30), (11, L30), (128, L30), (1, L30)], 2)]
    c["mul_pair_alias"] = c["mul_pair"]
    c["mul_pair_alias2"] = [([(64, L30), (2, L30), (1, L30), (64, L30)], 2)]           # x0 x1 and x1 x3: 128 each
    c["sqr_pair"] = [([(11, L30), (11, L30)], 2)]
    c["mul2"] = [([(8, L29)] * 4, 2), ([(64, L29), (1, L29), (32, L29), (2, L29)], 2), ([(6, L29), (10, L29), (2, L29), (34, L29)], 2)]
    c["mul2_mul_mul"] = [([(8, L29)] * 4 + [(64, L29), (2, L29), (2, L29), (64, L29)], 2),
                         ([(6, L29), (10, L29), (4, L29), (17, L29), (11, L29), (11, L29), (128, L29), (1, L29)], 2)]
    for n in range(1, 7):  # n products with sum(Ka Kb) <= 128
        c["mac%d" % n] = [([(128 // n, L29), (1, L29)] * n, 2), ([(1, L29), (128 // n, L29)] * n, 2)]
    for op, k in SUB_K.items():
        if op == "sub6_31":  # a limbs < 2^29, b < 6 p with limbs < 2^31 (the call sites: < 3 * 2^29)
            c[op] = [([(8, L29), (6, L31)], 14), ([(8, L29), (6, L3)], 14)]
        else:  # a limbs < 2^30 (any value the result can hold), b < K p with limbs < 2^30
            c[op] = [([(max(k, 64), L30), (k, L30)], max(k, 64) + k)]
    c["neg2"] = [([(2, L30)], 2)]
    c["neg4"] = [([(4, L30)], 4)]
    c["normalise"] = [([(128, L31)], 128)]
    c["reduced"] = [([(128, L29)], 2)]
    for op in ("canon", "to_mont256"):
        c[op] = [([(64, L29)], 1)]
    c["is_zero"] = [([(2, L29)], None)]
    c["pack"] = [([(W, L29)], None)]
    c["f2mul2"] = [([(32, L29), (32, L29), (2, L29), (2, L29)], 2)]                       # Ka Kb <= 64
    c["f2mul6"] = [([(10, L29), (10, L29), (6, L29), (6, L29)], 2)]
    c["f2sqr2"] = [([(2, L29), (2, L29)], 2)]
    c["f2sqr4"] = [([(4, L29), (4, L29)], 2)]
    c["f2mul2_42"] = [([(14, L29), (14, L29), (4, L29), (4, L29), (4, L29), (4, L29), (2, L29), (2, L29)], 2)]
    return c


def word_records(field, rng, n):
    """from_mont256 / unpack: operands are eight 32-bit words (any 256-bit value)"""
    recs = []
    edge = [0, 1, FIELDS[field][1] - 1, FIELDS[field][1], (1 << 256) - 1, sum(M29 << (29 * i) for i in range(8)) & ((1 << 256) - 1)]
    for v in edge + [rng.randrange(1 << 256) for _ in range(n)]:
        for op in ("from_mont256", "unpack"):
            recs.append(Rec(field, op, [words(v) + [0]], 2 if op == "from_mont256" else None, "contract"))
    return recs


def column_records(field, rng):
    """columns at their limits with no claim on the value: every limb of every operand maximal (2^29 - 1 for the
    normalised-operand forms, 2^30 - 1 for mul / sqr), exactness only"""
    recs = []
    m29 = [M29] * 9
    for n in range(1, 7):
        recs.append(Rec(field, "mac%d" % n, [m29] * (2 * n), None, "columns"))
    recs.append(Rec(field, "mul2", [m29] * 4, None, "columns"))
    recs.append(Rec(field, "mul2_mul_mul", [m29] * 8, None, "columns"))
    # limbs < 2^30 for mul / sqr: the top limb kept small enough that the output's fits 32 bits
    m30 = [L30 - 1] * 8 + [0]
    for op, ops in (("mul", [m30, m30]), ("sqr", [m30]), ("mul_pair", [m30] * 4), ("sqr_pair", [m30, m30])):
        recs.append(Rec(field, op, ops, None, "columns"))
    return recs


def build_records(seed=1, per_op=2000, table=None):
    """every contract edge, column stress and call-site row of `table`, plus `per_op` uniform records per operation and field"""
    rng = random.Random(seed)
    recs = []
    for op, cases in contracts().items():
        fields = ("q",) if op.startswith("f2") else ("q", "r")
        for field in fields:
            for specs, claim in cases:
                recs += case_records(field, op, specs, claim, "contract", rng)
                recs += random_records(field, op, specs, claim, "uniform", rng, max(1, per_op // len(cases)))
    for field in ("q", "r"):
        recs += word_records(field, rng, per_op // 4)
        recs += column_records(field, rng)
    for row in table or []:
        recs += case_records(row.field, row.op, row.specs, row.claim, row.site, rng)
    return recs


# ---- running the driver ------------------------------------------------------------------------------------------------
def build_host(tmp):
    exe = os.path.join(str(tmp), "field29_edges")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC, DRIVER, "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def build_device(tmp):
    import shutil

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(str(tmp), "field29_edges_gfx950")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "-I", CSRC, DRIVER, "-o", exe],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run(exe, recs, tmp, tag, timeout=300):
    fin = os.path.join(str(tmp), tag + ".in")
    fout = os.path.join(str(tmp), tag + ".out")
    encode(recs).tofile(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-1000:])
    out = np.fromfile(fout, dtype=np.uint32)
    assert out.size == len(recs) * REC_OUT
    return out.reshape(len(recs), REC_OUT)

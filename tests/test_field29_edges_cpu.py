"""The lazy 29-bit field arithmetic (csrc/field29.hpp, csrc/field2_29.hpp) at the edges of its bound contracts, on the host.

tests/host/field29_edges.cpp built with g++ runs every operation on operands at the edges of what its contract allows
(tests/field29_model.py: K p - 1 normalised and with every lower limb as large as allowed, 0, p, 2 p - 1, Ka Kb = 128
pairs, maximal six-product columns, seeded uniform values) and on every call site of SITES below at the bounds that call
site annotates.  Each output must be the exact result, the right value mod p, and meet the bound claimed for it.  The
gfx950 build of the same driver runs the same records in tests/test_field29_edges_gpu.py.
"""
import os
import re

import pytest

from tests import field29_model as M
from tests.field29_model import L29, L30, L31, L3, W

CSRC = M.CSRC


class Site:
    """one annotated call site: the source line it is on (found by `snippet`), the driver operation it amounts to, its
    operands' bounds as (K: value < K p -- or W, a memory word < 2^256 --, limb limit) and the bound it claims for the
    result (a multiple of p)"""

    def __init__(self, file, snippet, op, specs, claim, field):
        self.file, self.snippet, self.op, self.specs, self.claim, self.field = file, snippet, op, specs, claim, field
        self.site = "%s:%s" % (file, ",".join(str(n) for n in self.lines()))

    def lines(self):
        with open(os.path.join(CSRC, self.file)) as f:
            return [i + 1 for i, line in enumerate(f) if self.snippet in line]


def _n(*ks):  # normalised operands
    return [(k, L29) for k in ks]


def _f2(*ks):  # Fq2 operands, both components normalised and < K p
    return [(k, L29) for k in ks for _ in range(2)]


C1, C2, N, R = "curve29.hpp", "curve2_29.hpp", "ntt.hip", "poly.hip"
# file, snippet of the line, operation, operand bounds, claimed result bound.  Bounds as the code's comments state them.
TABLE = [
    # ---- curve29.hpp: G1 XYZZ on Fq29 (x < 8 p, y < 4 p, zz, zzz < 2 p) ----
    (C1, "r.x = Fq29::mul(r.x, f);", "mul", [(W, L29), (1, L29)], 2),                                    # load_affine29, mont256
    (C1, "r.y = Fq29::mul(r.y, f);", "mul", [(W, L29), (1, L29)], 2),
    (C1, "const Fq29 xr = v.x.reduced();", "reduced", _n(8), 2),                                           # store_xyzz29
    (C1, "const Fq29 red = F.reduced();", "reduced", _n(8), 2),                                            # quad_store (lane 0: x)
    (C1, "const Fq29 v = u.sqr();                      // 16", "sqr", [(4, L30)], 2),                       # dbl_affine, u = y + y
    (C1, "const Fq29 w = u * v;                        // 8", "mul", [(4, L30), (2, L29)], 2),
    (C1, "const Fq29 s = a.x * v;", "mul", _n(2, 2), 2),
    (C1, "const Fq29 x2 = a.x.sqr();", "sqr", _n(2), 2),
    (C1, "Fq29::sub<4>(m.sqr(), s + s);", "sqr", _n(6), 2),                                                # m < 6
    (C1, "Fq29::sub<4>(m.sqr(), s + s);", "sub4", [(2, L29), (4, L30)], 6),                                # s + s < 4, limbs < 2^30
    (C1, "w, Fq29::neg<2>(a.y));  // m (s - x3) - w y", "sub8", _n(2, 8), 10),
    (C1, "w, Fq29::neg<2>(a.y));  // m (s - x3) - w y", "neg2", _n(2), 2),
    (C1, "w, Fq29::neg<2>(a.y));  // m (s - x3) - w y", "mul2", _n(6, 10, 2, 2), 2),                         # 64
    (C1, "const Fq29 v = u.sqr();                      // 64", "sqr", [(8, L30)], 2),                       # dbl, u = y + y < 8
    (C1, "const Fq29 w = u * v;                        // 16", "mul", [(8, L30), (2, L29)], 2),
    (C1, "const Fq29 s = p.x * v;", "mul", _n(8, 2), 2),
    (C1, "const Fq29 x2 = p.x.sqr();", "sqr", _n(8), 2),
    (C1, "w, Fq29::neg<4>(p.y));  // 6 * 10 + 2 * 4 = 68", "neg4", _n(4), 4),
    (C1, "w, Fq29::neg<4>(p.y));  // 6 * 10 + 2 * 4 = 68", "mul2", _n(6, 10, 2, 4), 2),
    (C1, "return {x3, y3, v * p.zz, w * p.zzz};", "mul", _n(2, 2), 2),
    (C1, "Fq29::mul_pair(a.x, acc.zz, a.y, acc.zzz, u2, s2);", "mul_pair", _n(2, 2, 2, 2), 2),           # add_affine
    (C1, "const Fq29 p = Fq29::sub<8>(u2, acc.x);", "sub8", _n(2, 8), 10),
    (C1, "const Fq29 r = Fq29::sub<4>(s2, acc.y);", "sub4", _n(2, 4), 6),
    (C1, "Fq29::sqr_pair(p, r, pp, rr);                // 100, 36", "sqr_pair", _n(10, 6), 2),
    (C1, "Fq29::mul_pair(p, pp, acc.x, pp, ppp, q);", "mul_pair", _n(10, 2, 8, 2), 2),
    (C1, "Fq29::sub<6, 31>(rr, ppp + q + q);                    // subtrahend", "sub6_31", [(2, L29), (6, L3)], 8),
    (C1, "Fq29::mul2_mul_mul(r, Fq29::sub<8>(q, x3), Fq29::neg<4>(acc.y)", "sub8", _n(2, 8), 10),
    (C1, "Fq29::mul2_mul_mul(r, Fq29::sub<8>(q, x3), Fq29::neg<4>(acc.y)", "neg4", _n(4), 4),
    (C1, "Fq29::mul2_mul_mul(r, Fq29::sub<8>(q, x3), Fq29::neg<4>(acc.y)", "mul2_mul_mul", _n(6, 10, 4, 2, 2, 2, 2, 2), 2),
    (C1, "Fq29::mul_pair(acc.x, b.zz, b.x, acc.zz, u1, u2);", "mul_pair", _n(8, 2, 8, 2), 2),            # add
    (C1, "Fq29::mul_pair(acc.y, b.zzz, b.y, acc.zzz, s1, s2);", "mul_pair", _n(4, 2, 4, 2), 2),
    (C1, "const Fq29 p = Fq29::sub<2>(u2, u1);", "sub2", _n(2, 2), 4),
    (C1, "const Fq29 r = Fq29::sub<2>(s2, s1);", "sub2", _n(2, 2), 4),
    (C1, "Fq29::sqr_pair(p, r, pp, rr);                // 16, 16", "sqr_pair", _n(4, 4), 2),
    (C1, "Fq29::mul_pair(p, pp, u1, pp, ppp, q);", "mul_pair", _n(4, 2, 2, 2), 2),
    (C1, "Fq29::mul_pair(acc.zz, b.zz, acc.zzz, b.zzz, zz, zzz);", "mul_pair", _n(2, 2, 2, 2), 2),
    (C1, "Fq29::sub<6, 31>(rr, ppp + q + q);                   // x3 < 8", "sub6_31", [(2, L29), (6, L3)], 8),
    (C1, "Fq29::mul2(r, Fq29::sub<8>(q, x3), Fq29::neg<2>(s1), ppp);", "sub8", _n(2, 8), 10),
    (C1, "Fq29::mul2(r, Fq29::sub<8>(q, x3), Fq29::neg<2>(s1), ppp);", "neg2", _n(2), 2),
    (C1, "Fq29::mul2(r, Fq29::sub<8>(q, x3), Fq29::neg<2>(s1), ppp);", "mul2", _n(4, 10, 2, 2), 2),        # 44
    (C1, "Fq29::mul_pair(zz, pp, zzz, ppp, acc.zz, acc.zzz);", "mul_pair", _n(2, 2, 2, 2), 2),
    (C1, "return {(v.x * v.zz).to_mont256(), (v.y * v.zzz).to_mont256(), v.zz.to_mont256()};", "mul", _n(8, 2), 2),
    (C1, "return {(v.x * v.zz).to_mont256(), (v.y * v.zzz).to_mont256(), v.zz.to_mont256()};", "to_mont256", _n(2), 1),
    (C1, "const Fq29 T1 = Fq29::mul(A1, B1);", "mul", _n(8, 2), 2),                                       # quad_add
    (C1, "const Fq29 D = Fq29::sub<2>(quad_perm<1, 3, 1, 3>(T1)", "sub2", _n(2, 2), 4),
    (C1, "const Fq29 T2 = Fq29::mul(select29(role < 2, D, F)", "mul", _n(4, 4), 2),
    (C1, "const Fq29 T3 = Fq29::mul(role == 0 ? D : role == 1 ? U1 : T2, PP);", "mul", _n(4, 2), 2),
    (C1, "const Fq29 X3 = Fq29::sub<6, 31>(T2, PPP + T3 + T3);", "sub6_31", [(2, L29), (6, L3)], 8),
    (C1, "const Fq29 W = Fq29::sub<8>(T3, X3);", "sub8", _n(2, 8), 10),
    (C1, "const Fq29 T4 = Fq29::mul(role == 0 ? S1", "mul", _n(4, 10), 2),
    (C1, "const Fq29 Y3 = Fq29::sub<2>(T4, quad_perm<0, 0, 0, 0>(T4));", "sub2", _n(2, 2), 4),
    # ---- curve2_29.hpp: G2 XYZZ on Fq2_29 (every component < 2 p) ----
    (C2, "c[k] = Fq29::mul(Fq29::unpack(w), f);", "mul", [(W, L29), (1, L29)], 2),                      # load_affine2_29
    (C2, "const F2 v = u.sqr<4>();", "f2sqr4", _f2(4), 2),                                                # u = y + y < 4
    (C2, "const F2 w = F2::mul<2>(u, v);", "f2mul2", _f2(4, 2), 2),
    (C2, "const F2 s = F2::mul<2>(a.x, v);", "f2mul2", _f2(2, 2), 2),
    (C2, "const F2 s = F2::mul<2>(p.x, v);", "f2mul2", _f2(2, 2), 2),
    (C2, "const F2 x2 = a.x.sqr<2>();", "f2sqr2", _f2(2), 2),
    (C2, "const F2 x2 = p.x.sqr<2>();", "f2sqr2", _f2(2), 2),
    (C2, "F2::sub<4>(F2::mul<6>(m, m), s + s).reduced();", "f2mul6", _f2(6, 6), 2),                      # 72
    (C2, "F2::sub<4>(F2::mul<6>(m, m), s + s).reduced();", "sub4", [(2, L29), (4, L30)], 6),
    (C2, "F2::sub<4>(F2::mul<6>(m, m), s + s).reduced();", "reduced", _n(6), 2),
    (C2, "F2::mul2<4, 2>(m, F2::sub<2>(s, x3), w, F2::neg<2>(a.y));", "sub2", _n(2, 2), 4),
    (C2, "F2::mul2<4, 2>(m, F2::sub<2>(s, x3), w, F2::neg<2>(a.y));", "neg2", _n(2), 2),
    (C2, "F2::mul2<4, 2>(m, F2::sub<2>(s, x3), w, F2::neg<2>(a.y));", "f2mul2_42", _f2(6, 4, 2, 2), 2),   # 56
    (C2, "F2::mul2<4, 2>(m, F2::sub<2>(s, x3), w, F2::neg<2>(p.y));", "f2mul2_42", _f2(6, 4, 2, 2), 2),
    (C2, "return {x3, y3, F2::mul<2>(v, p.zz), F2::mul<2>(w, p.zzz)};", "f2mul2", _f2(2, 2), 2),
    (C2, "const F2 u2 = F2::mul<2>(a.x, acc.zz);", "f2mul2", _f2(2, 2), 2),                              # add_affine
    (C2, "const F2 s2 = F2::mul<2>(a.y, acc.zzz);", "f2mul2", _f2(2, 2), 2),
    (C2, "const F2 p = F2::sub<2>(u2, acc.x);", "sub2", _n(2, 2), 4),
    (C2, "const F2 r = F2::sub<2>(s2, acc.y);", "sub2", _n(2, 2), 4),
    (C2, "const F2 pp = p.sqr<4>();", "f2sqr4", _f2(4), 2),
    (C2, "const F2 rr = r.sqr<4>();", "f2sqr4", _f2(4), 2),
    (C2, "const F2 ppp = F2::mul<2>(p, pp);", "f2mul2", _f2(4, 2), 2),
    (C2, "const F2 q = F2::mul<2>(acc.x, pp);", "f2mul2", _f2(2, 2), 2),
    (C2, "const F2 x3 = F2::sub<6, 31>(rr, ppp + q + q).reduced();", "sub6_31", [(2, L29), (6, L3)], 8),
    (C2, "const F2 x3 = F2::sub<6, 31>(rr, ppp + q + q).reduced();", "reduced", _n(8), 2),
    (C2, "F2::mul2<4, 2>(r, F2::sub<2>(q, x3), F2::neg<2>(acc.y), ppp);", "f2mul2_42", _f2(4, 4, 2, 2), 2),  # 40
    (C2, "acc.zz = F2::mul<2>(acc.zz, pp);", "f2mul2", _f2(2, 2), 2),
    (C2, "acc.zzz = F2::mul<2>(acc.zzz, ppp);", "f2mul2", _f2(2, 2), 2),
    (C2, "const F2 u1 = F2::mul<2>(acc.x, b.zz);", "f2mul2", _f2(2, 2), 2),                              # add
    (C2, "const F2 u2 = F2::mul<2>(b.x, acc.zz);", "f2mul2", _f2(2, 2), 2),
    (C2, "const F2 s1 = F2::mul<2>(acc.y, b.zzz);", "f2mul2", _f2(2, 2), 2),
    (C2, "const F2 s2 = F2::mul<2>(b.y, acc.zzz);", "f2mul2", _f2(2, 2), 2),
    (C2, "const F2 r = F2::sub<2>(s2, s1);", "sub2", _n(2, 2), 4),
    (C2, "const F2 q = F2::mul<2>(u1, pp);", "f2mul2", _f2(2, 2), 2),
    (C2, "acc.zzz = F2::mul<2>(F2::mul<2>(acc.zzz, b.zzz), ppp);", "f2mul2", _f2(2, 2), 2),
    (C2, "const F2 p = F2::sub<2>(u2, u1);", "sub2", _n(2, 2), 4),
    (C2, "const F2 ppp = F2::mul<2>(p, pp);", "f2mul2", _f2(4, 2), 2),
    (C2, "F2::mul2<4, 2>(r, F2::sub<2>(q, x3), F2::neg<2>(s1), ppp);", "neg2", _n(2), 2),
    (C2, "F2::mul2<4, 2>(r, F2::sub<2>(q, x3), F2::neg<2>(s1), ppp);", "f2mul2_42", _f2(4, 4, 2, 2), 2),
    (C2, "acc.zz = F2::mul<2>(F2::mul<2>(acc.zz, b.zz), pp);", "f2mul2", _f2(2, 2), 2),
    (C2, "return {to_mont256_2(F2::mul<2>(v.x, v.zz))", "f2mul2", _f2(2, 2), 2),
    (C2, "return {to_mont256_2(F2::mul<2>(v.x, v.zz))", "to_mont256", _n(2), 1),
    # ---- ntt.hip: level r holds values < B_r p, B_r = 2^(r+1) <= 64 ----
    (N, "case 0: return Fr29::sub<2>(u, v);", "sub2", [(2, L30), (2, L30)], 4),                          # sub_level: a, b < K p
    (N, "case 1: return Fr29::sub<4>(u, v);", "sub4", [(4, L30), (4, L30)], 8),                          # (limbs < 2^30: the
    (N, "case 2: return Fr29::sub<8>(u, v);", "sub8", [(8, L30), (8, L30)], 16),                         # radix-4 step's sums)
    (N, "case 3: return Fr29::sub<16>(u, v);", "sub16", [(16, L30), (16, L30)], 32),
    (N, "case 4: return Fr29::sub<32>(u, v);", "sub32", [(32, L30), (32, L30)], 64),
    (N, "default: return Fr29::sub<64>(u, v);", "sub64", [(64, L30), (64, L30)], 128),
    (N, "g_store29(t + j, Fr29::mul(g_load29(t + j), const29(CONSTS29<FrP>.from256)), true);", "mul", [(W, L29), (1, L29)], 2),
    (N, "cl = Fr29::mul(Fr29::unpack(a.in_coset[threadIdx.x - 1].v.l), const29(CONSTS29<FrP>.c271));", "mul", [(W, L29), (1, L29)], 2),
    (N, "x = Fr29::mul(x, lds_load29(cl29 + (g % 3) * 9, 1, 0));", "mul", [(W, L29), (2, L29)], 2),
    (N, "if (dj) Fr29::mul_pair(d02, lds_load29(tw29, half, dj << rnd), d13,", "mul_pair_alias", _n(64, 1, 64, 1), 2),
    (N, "else d13 = Fr29::mul(d13, lds_load29(tw29, half, (dj + hb) << rnd));", "mul", _n(64, 1), 2),
    (N, "Fr29 y0 = s02 + s13;                      // < 4 B_r p", "normalise", [(128, L31)], 128),
    (N, "Fr29::mul_pair(y1, w2, y3, w2, y1, y3);  // 4 B_r * 1 <= 128", "mul_pair_alias", _n(128, 1, 128, 1), 2),
    (N, "if (di) d = Fr29::mul(d, lds_load29(tw29, half, di << rnd));", "mul", _n(128, 1), 2),           # generic: 2 B_5 = 128
    (N, "if (h) w = canon29(Fr29::mul(w, g_load29(a.tw_hi + h)));", "mul", _n(1, 1), 2),
    (N, "Fr29::mul_pair(xa, wa, xb, wb, ra, rb);  // 128 * 1", "mul_pair", _n(128, 1, 128, 1), 2),
    (N, "if (di) d = Fr29::mul(d, lds_load29(tw29, half, di << rnd));", "mul", _n(128, 1), 2),
    # ---- poly.hip: memory words (W) read as limbs, R' constants < p ----
    (R, "acc = Fr29::mul(acc, x256) + cf;  // < 3 p, limbs < 2^30", "mul", [(3, L30), (1, L29)], 2),     # block_eval
    (R, "if ((t >> bit) & 1u) acc = Fr29::mul(acc, Fr29::unpack(pw.sq[bit].v.l));", "mul", _n(3, 1), 2),
    (R, "acc.to_canonical_words(w);", "canon", _n(14), 1),                                                # lincomb: 7 groups < 2 p
    (R, "Fr29::mac(col, Fr29::unpack(w), c);", "mac6", [(W, L29), (1, L29)] * 6, 2),                       # lincomb, 6 per redc
    (R, "acc = acc + Fr29::redc(col);  // < 2 p each", "mac6", [(W, L29), (1, L29)] * 6, 2),
    (R, "Fr29 w = Fr29::mul(f, la) + beta;  // < 3 p, limbs < 2^30", "mul", [(W, L29), (W, L29)], 2),     # cq_quotient
    (R, "Fr29::mac(col, acc, y);   // acc < 4 p", "mac2", [(4, L29), (1, L29), (W, L29), (3, L29)], 2),
    (R, "Fr29::mac(col, b, w);", "mac2", [(4, L29), (1, L29), (W, L29), (3, L29)], 2),                    # (with the line above)
    (R, "acc = Fr29::sub<2>(Fr29::redc(col), one);  // < 4 p", "sub2", _n(2, 1), 4),
    (R, "if (args.h_in) acc = Fr29::mul(load29(args.h_in + i), Fr29::unpack(k.c_1024.v.l));", "mul", [(W, L29), (1, L29)], 2),
    (R, "acc = Fr29::mul(acc, Fr29::unpack(k.scale261.v.l));", "mul", _n(4, 1), 2),
    (R, "if (args.t_len) acc = Fr29::mul(acc, load29(args.t_evals", "mul", [(2, L29), (W, L29)], 2),
    (R, "Fr29::mul_pair(acc_a, elem(k), acc_b, elem(k + H), acc_a, acc_b);", "mul_pair_alias", [(2, L29), (W, L29)] * 2, 2),
    (R, "const Fr29 acc = Fr29::mul(acc_a, acc_b);", "mul", _n(2, 2), 2),                                 # batch inversion
    (R, "Fr29::mul_pair(below, inc, suf, above, inc, suf);", "mul_pair", [(W, L29)] * 4, 2),
    (R, "const Fr29 exc_b = Fr29::mul(exc, total_a);", "mul", [(W, L29), (2, L29)], 2),
    (R, "Fr29 r = Fr29::mul(total_inv, after);", "mul", [(W, L29), (W, L29)], 2),
    (R, "Fr29::mul_pair(k1 >= H ? exc_b : exc, prefix(k1), k0 >= H ? exc_b : exc, prefix(k0), b1, b0);", "mul_pair", _n(2, 2, 2, 2), 2),
    (R, "Fr29::mul_pair(b1, r, r, elem(k1), o1, r);", "mul_pair_alias2", [(2, L29), (2, L29), (2, L29), (W, L29)], 2),
    (R, "Fr29::mul_pair(b0, r, r, elem(k0), o0, r);", "mul_pair_alias2", [(2, L29), (2, L29), (2, L29), (W, L29)], 2),
]
SITES = [Site(f, s, op, specs, claim, "q" if f in (C1, C2) else "r") for f, s, op, specs, claim in TABLE]

# lines of these files that call a bounded operation; every one must be some row's line (but the canonical Fr's squarings
# of the host-side powers in poly.hip, which are not lazy values)
_NOT_LAZY = {(R, "y = y.sqr();")}
_CALL = re.compile(r"(Fq29|Fr29|F2)::(mul|mul2|mul_pair|sqr_pair|mul2_mul_mul|sub|neg|mac|redc|mul<|mul2<)\b|\.sqr(<\d+>)?\(\)|\.reduced\(\)"
                   r"|\b(u|a\.x|p\.x|v|w|v\.x|v\.y) \* (v|p\.zz|p\.zzz|v\.zz|v\.zzz)\b|to_canonical_words\(")


def test_call_site_table_covers_every_bounded_call():
    """Every row's snippet is on a line of its file, and every line of curve29.hpp, curve2_29.hpp, ntt.hip and poly.hip that
    calls a bounded Fp29 / Fq2_29 operation on lazy values is some row's line: the table is the complete list of annotated
    bounds, and a changed call site fails here until its row follows."""
    missing = [(s.file, s.snippet) for s in SITES if not s.lines()]
    assert not missing, missing
    covered = {(s.file, n) for s in SITES for n in s.lines()}
    uncovered = []
    for f in (C1, C2, N, R):
        with open(os.path.join(CSRC, f)) as fh:
            for i, line in enumerate(fh):
                code = line.split("//")[0]
                if any(f == nf and sn in line for nf, sn in _NOT_LAZY):
                    continue
                if _CALL.search(code) and (f, i + 1) not in covered:
                    uncovered.append("%s:%d: %s" % (f, i + 1, line.strip()))
    assert not uncovered, "\n".join(uncovered)


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("field29")
    recs = M.build_records(seed=1, per_op=2000, table=SITES)
    exe = M.build_host(tmp)
    return recs, M.run(exe, recs, tmp, "host")


def test_field29_edges_host_exact_and_within_bounds(host_run):
    """Every record (contract edges, maximal columns, uniform operands, the call-site rows) gives the exact result, the
    right value mod p, normalised limbs and a value within the claimed bound."""
    recs, out = host_run
    assert len(recs) > 50000
    bad = M.check(recs, out)
    assert not bad, "\n".join(bad[:40])


def test_field29_call_sites_at_their_extremes(host_run):
    """Each row of the call-site table ran at its extreme operands (every operand at K p - 1, normalised and spread where
    the call site allows) and passed."""
    recs, out = host_run
    srcs = {r.src for r in recs}
    for s in SITES:
        assert s.site in srcs, s.site
    rows = [i for i, r in enumerate(recs) if r.src not in ("contract", "uniform", "columns")]
    bad = M.check([recs[i] for i in rows], out[rows])
    assert not bad, "\n".join(bad[:40])

"""CPU model of the MSM's signed-digit recoding (msm_sort.hip: signed_digit) and of which sorting front a launch takes
(MsmLayout::part_sort / mid, part_shift_of, msm_multi_begin's cut-over to the short kernel), plus the crafted scalars the
edge tests feed to every front: each family is built for ONE digit event (a digit exactly M, a zero digit that still
carries, a carry chain into the top window, ...).  tests/test_msm_digits_cpu.py holds the model to the events, and
tests/test_msm_edges_gpu.py runs the families through the kernels against the C oracle.

The constants are read from the sources, so a change of a threshold there shows up in the CPU test's routing table."""
import os
import re
from collections import OrderedDict

from oracle import bn254 as B

R = B.R_MOD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(ROOT, "sha2_on_cq_halo2_amd", "csrc")
_HPP = open(os.path.join(_CSRC, "msm.hpp")).read()
_HIP = open(os.path.join(_CSRC, "msm.hip")).read()            # msm_window_bits; the overview quotes the layout's routing lines
_SORT = open(os.path.join(_CSRC, "msm_sort.hip")).read()      # the partition front and its specialisations
_LAYOUT = open(os.path.join(_CSRC, "msm_layout.hpp")).read()  # MsmLayout: what routes a launch to a front


def _shift_const(text, name):
    """`NAME = 1u << K` -> 2^K"""
    return 1 << int(re.search(r"\b%s = 1u << (\d+)" % name, text).group(1))


def routing_constants(text):
    """(PSC_MAX_WIN, PART_BITS, PART_BITS_WIDE, DIGITS_LDS_MAX_M, REFINE_ABOVE, REFINE_SHIFT, WIDE_ABOVE, MID_ABOVE) as `text` states them:
    part_shift_of(c): c > REFINE_ABOVE ? c - REFINE_SHIFT : c > WIDE_ABOVE ? PART_BITS_WIDE : PART_BITS;
    MsmLayout: mid = part_sort && c > MID_ABOVE"""
    m = re.search(r"part_shift_of\(uint32_t c\) \{ return c > (\d+) \? c - (\d+) : c > (\d+) \? PART_BITS_WIDE : PART_BITS; \}", text)
    return (int(re.search(r"PSC_MAX_WIN = (\d+)", text).group(1)), int(re.search(r"\bPART_BITS = (\d+)", text).group(1)),
            int(re.search(r"\bPART_BITS_WIDE = (\d+)", text).group(1)), _shift_const(text, "DIGITS_LDS_MAX_M")) + tuple(int(g) for g in m.groups()) + (
                int(re.search(r"mid = part_sort && c > (\d+);", text).group(1)),)


MSM_SHORT_MAX = int(re.search(r"#define CQ_MSM_SHORT_MAX (\d+)", _HPP).group(1))
MSM_TABLE_C_MIN = int(re.search(r"MSM_TABLE_C_MIN = (\d+)", _HPP).group(1))
MSM_TABLE_C_MAX = int(re.search(r"MSM_TABLE_C_MAX = (\d+)", _HPP).group(1))
PSC_MAX_WIN, PART_BITS, PART_BITS_WIDE, DIGITS_LDS_MAX_M, REFINE_ABOVE, REFINE_SHIFT, WIDE_ABOVE, MID_ABOVE = routing_constants(_LAYOUT)
# the (c, W) pairs whose first partition pass has the window width and count as compile-time constants
PART_SPECIALISED = [(int(a), int(b)) for a, b in re.findall(r"launch_part_pass1<(\d+), (\d+), uint\d+_t>", _SORT) if int(a)]
# msm_window_bits(n): [(threshold, c)], largest threshold first, and the width below the last one
_body = re.search(r"uint32_t msm_window_bits\(uint32_t n\) \{(.*?)\n\}", _HIP, re.S).group(1)
WINDOW_BITS = [((1 << int(s)) if s else int(v), int(c)) for s, v, c in
               re.findall(r"if \(n >= (?:\(1u << (\d+)\)|(\d+))\) return (\d+);", _body)]
WINDOW_BITS_MIN = int(re.search(r"\n  return (\d+);", _body).group(1))


def windows(c):
    """W = ceil(255 / c): signed digits need W * c >= 255 for 254-bit scalars"""
    return (255 + c - 1) // c


def digits(v, c):
    """signed_digit over every window of the canonical scalar v: the W signed digits (each in -(M-1) .. M) and the carry
    left after the last window"""
    M = 1 << (c - 1)
    out, carry = [], 0
    for w in range(windows(c)):
        raw = (v >> (c * w)) & ((1 << c) - 1) if c * w < 256 else 0
        d = raw + carry
        carry = 0
        if d > M:  # M itself stays positive: the last bucket
            d = d - (1 << c)
            carry = 1
        out.append(d)
    return out, carry


def carries_on_zero(v, c):
    """windows whose digit is zero although they pass a carry on (raw + carry = 2^c)"""
    carry, hits = 0, 0
    for w in range(windows(c)):
        raw = (v >> (c * w)) & ((1 << c) - 1)
        d = raw + carry
        carry = 1 if d > (1 << (c - 1)) else 0
        hits += d == (1 << c)
    return hits


def window_bits(n):
    """msm_window_bits: the plain pipeline's window width for n terms"""
    for threshold, c in WINDOW_BITS:
        if n >= threshold:
            return c
    return WINDOW_BITS_MIN


def plain_path(n, forced_c=0):
    """msm_multi_begin, no tables registered: ("short", 8) up to MSM_SHORT_MAX terms unless the caller fixed the window,
    else the generic pipeline with the forced or the automatic width"""
    if not forced_c and n <= MSM_SHORT_MAX:
        return "short", 8
    return front_of(False, forced_c or window_bits(n)), forced_c or window_bits(n)


def front_of(pre, c):
    """Which kernels turn scalars into sorted bucket lists in msm_run:
    "digits"       msm_digits_kernel + msm_scatter_kernel (plain mode; table mode with more windows than PSC_MAX_WIN)
    "part"         msm_part_hist / msm_part_scatter, 2^PART_BITS buckets per partition
    "part-wide"    ... 2^PART_BITS_WIDE buckets per partition
    "part-refine"  ... 2^(c - REFINE_SHIFT) buckets per partition, then the refinement pass down to 2^PART_BITS"""
    if not pre:
        return "digits"
    buckets = 1 << (c - 1)
    part_sort = (buckets <= DIGITS_LDS_MAX_M << (MSM_TABLE_C_MAX - 15)) and buckets >= (1 << PART_BITS) and windows(c) <= PSC_MAX_WIN
    if not part_sort:
        return "digits"
    if c > MID_ABOVE:
        assert c > REFINE_ABOVE
        return "part-refine"
    return "part-wide" if c > WIDE_ABOVE else "part"


def below_top(c):
    """J: the number of windows strictly below the one holding bit 253 (the top bit of r)"""
    return 253 // c


def single(c, w, d):
    return d << (c * w)


def cancel(c, w, d):
    """(a, b): on one base, +d and -d at window w (P_w and -P_w in bucket d - 1) and a lone +1 at window w + 1"""
    a = d << (c * w)
    return a, (1 << (c * (w + 1))) - a


def single_keys(c):
    """every (w, d), d in {1, M - 1, M}, whose scalar d * 2^(cw) is below r"""
    M = 1 << (c - 1)
    ds = sorted({1, M - 1, M} - {0})
    return [(w, d) for w in range(windows(c)) for d in ds if single(c, w, d) < R]


def cancel_keys(c):
    """(w, d) for d in {1, M - 1} (d = M does not cancel: b would equal a) and w in {0, a middle window, the last below the top}"""
    M = 1 << (c - 1)
    J = below_top(c)
    return [(w, d) for w in sorted({0, J // 2, J - 1}) for d in sorted({1, M - 1})]


CONSTANTS = OrderedDict([("0", 0), ("1", 1), ("2", 2), ("r-1", R - 1), ("r-2", R - 2), ("2^253+1", (1 << 253) + 1), ("2^128-1", (1 << 128) - 1)]
                        + [("2^%d-1" % (32 * j), (1 << (32 * j)) - 1) for j in range(1, 8)]
                        + [("2^%d" % (32 * j), 1 << (32 * j)) for j in range(1, 8)])


def edge_scalars(c):
    """name -> tuple of canonical scalars below r, each family built for one digit event of c-bit windows"""
    M = 1 << (c - 1)
    J = below_top(c)
    fam = OrderedDict()
    fam["all_M"] = (sum(M << (c * w) for w in range(J)),)
    fam["all_M_plus_1"] = (sum((M + 1) << (c * w) for w in range(J)),)
    fam["all_full"] = ((1 << (c * J)) - 1,)
    fam["one_then_M_minus_1"] = ((M + 1) + ((M - 1) << c),)
    for w, d in single_keys(c):
        fam["single(%d,%d)" % (w, d)] = (single(c, w, d),)
    for w, d in cancel_keys(c):
        fam["cancel(%d,%d)" % (w, d)] = cancel(c, w, d)
    for name, v in CONSTANTS.items():
        fam["const:" + name] = (v,)
    return fam


def edge_values(c):
    """the families of edge_scalars(c), flattened in order"""
    return [v for vals in edge_scalars(c).values() for v in vals]

"""CPU side of the trapdoor-free setup path: the ABI lists its entry points, and the signed-digit recoding that the
fixed-window G1 FFT relies on (csrc/g1window.hpp) is exact -- a host build of the very header, under AddressSanitizer and
UBSan, against Python integers."""
import os
import subprocess

import numpy as np

from oracle import bn254 as B
from oracle.poly import EvaluationDomain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = B.R_MOD
SYMBOLS = ["cq_params_from_powers", "cq_table_config_from_srs", "cq_static_table_new_fk_dev", "cq_g_to_lagrange_windowed_dev"]
DIGITS, W = 85, 3


def test_header_and_rust_bindings_list_the_entry_points():
    from sha2_on_cq_halo2_amd import _lib

    protos = {p.name: p for p in _lib.header_prototypes()}
    rs = open(os.path.join(ROOT, "include", "cq_halo2_sys.rs")).read()
    for name in SYMBOLS:
        assert name in protos, name
        assert "pub fn %s(" % name in rs, name
    assert protos["cq_params_from_powers"].params == ["cq_ctx* ctx", "uint32_t k", "const uint64_t* g", "int g_on_device", "cq_params** out"]
    assert protos["cq_table_config_from_srs"].params == ["cq_ctx* ctx", "size_t size", "const uint64_t* srs_g1", "size_t srs_len",
                                                         "int on_device", "cq_table_config** out"]
    assert protos["cq_static_table_new_fk_dev"].params == ["cq_ctx* ctx", "size_t size", "const uint64_t* values",
                                                           "const uint64_t* srs_g1_dev", "cq_static_table** out"]


def _from_digits(ds):
    return sum(d << (W * i) for i, d in enumerate(ds))


def _scalars():
    """0, 1, r - 1 and their neighbours; every digit at one extreme, at the other, alternating, and one digit at an extreme
    among ones (odd m, and the even k = r - m that recodes to the same m); every twiddle of a 2^10 domain, w and 1/w; random."""
    out = [0, 1, 2, 3, R - 1, R - 2, R - 3, (R - 1) // 2, (R + 1) // 2, (1 << 253) - 1, 1 << 253]
    top = [1, 3]  # the top digit of an m < 2^254
    shapes = []
    for t in top:
        shapes.append([7] * (DIGITS - 1) + [t])
        shapes.append([-7] * (DIGITS - 1) + [t])
        shapes.append([7 if i % 2 else -7 for i in range(DIGITS - 1)] + [t])
        shapes.append([-7 if i % 2 else 7 for i in range(DIGITS - 1)] + [t])
        for pos in range(DIGITS - 1):
            for e in (7, -7):
                d = [1] * (DIGITS - 1) + [t]
                d[pos] = e
                shapes.append(d)
    for d in shapes:
        m = _from_digits(d)
        assert m % 2 == 1 and m > 0
        if m < R:
            out += [m, R - m]
    assert len(out) > 300
    w = EvaluationDomain(2, 10).omega
    cur = 1
    for _ in range(1 << 10):
        out += [cur, B.inv_mod(cur, R)]
        cur = cur * w % R
    rng = B.Xoshiro256ss(0x6731)
    out += [B.fr_random(rng) for _ in range(500)]
    return out


def test_g1window_recoding_matches_python_integers(tmp_path):
    exe = str(tmp_path / "g1window_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-Wall", "-Wextra", "-Werror",
                        "-I", os.path.join(ROOT, "sha2_on_cq_halo2_amd", "csrc"), os.path.join(ROOT, "tests", "host", "g1window_check.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    ks = _scalars()
    assert all(0 <= k < R for k in ks)
    fin, fout = str(tmp_path / "in"), str(tmp_path / "out")
    np.array([[(k >> (32 * i)) & 0xFFFFFFFF for i in range(8)] for k in ks], dtype=np.uint32).tofile(fin)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr[-3000:]
    rec = np.fromfile(fout, dtype=np.uint32).reshape(len(ks), 9 + 3 * DIGITS)
    seen = set()
    for k, o in zip(ks, rec):
        m = k if k & 1 else R - k
        assert int(o[8]) == (0 if k & 1 else 1), hex(k)
        c = sum(int(x) << (32 * i) for i, x in enumerate(o[:8]))
        assert c == (m >> 1) + (1 << 254), hex(k)
        v = [int(x) for x in o[9::3]]
        assert v == [(c >> (W * i)) & 7 for i in range(DIGITS)], hex(k)
        digits = [2 * x - 7 for x in v]
        assert _from_digits(digits) == m, hex(k)          # odd digits in [-7, 7] that spell m: no zero digit by construction
        assert digits[-1] in (1, 3), hex(k)               # the chain starts from a positive table entry
        sign = -1 if o[8] else 1
        assert sign * m % R == k, hex(k)                  # (r - k) P = -k P
        for x, idx, neg in zip(v, o[10::3], o[11::3]):    # table index (|d| - 1) / 2 and sign
            d = 2 * x - 7
            assert int(idx) == (abs(d) - 1) // 2 and int(neg) == (1 if d < 0 else 0)
        seen.update(digits[:-1])
    assert seen == {-7, -5, -3, -1, 1, 3, 5, 7}

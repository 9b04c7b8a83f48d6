"""Load-time figures of a serialized G2 SRS (the G2 leg next to tools/serde_perf.py): wall time of cq_g2_srs_read in
SerdeFormat::Processed and in checked RawBytes, of cq_g2_srs_create(checked = 1) from host points (the host loop the GPU
validation replaces), the decompression kernel's own time (HIP events, CQ_PROF_G2_DECOMPRESS), and the chip's Fq product
rate from the same run (cq_bench_modmul_dev, lazy 29-bit form) -- so that the kernel can be held against
    products per point x points / measured product rate,
the figure DESIGN 9a gives for G1.

usage: python tools/serde_g2_perf.py [log2(count) ...]      (default: 16 18)
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sha2_on_cq_halo2_amd import Context, G2Srs
from sha2_on_cq_halo2_amd.api import PROF_G2_DECOMPRESS, SERDE_PROCESSED, SERDE_RAW_BYTES, fr_to_mont
from tools.serde_perf import modmul_rate

# csrc/sqrt2_29.hpp (W = 4) and g2_decompress_kernel.  The root: a0 and a1 reduced, the norm (two products, one reduction),
# two chains of 14 table entries + 4 squarings for each of the 62 digits below the top one + a product for each non-zero one,
# s^2 and its reduced difference, the two halvings and a1 / 2, c, c^2, its reduced difference, a1 w / 2 and its reduced
# negation, y.c0 out of Montgomery form.  Around it: x to the limb form (2) and to the memory form (2), x^2 (2), x^3 (4),
# y to the memory form (2).
Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47


def _chain(e):
    digits = [(e >> (4 * j)) & 15 for j in range(64)]
    top = max(j for j, d in enumerate(digits) if d)
    return 14 + 4 * top + sum(1 for d in digits[:top] if d)


ROOT_PRODUCTS = 2 + 2 + _chain((Q + 1) // 4) + 2 + 3 + _chain((Q - 3) // 4) + 5 + 1
PRODUCTS_PER_POINT = ROOT_PRODUCTS + 2 + 2 + 2 + 4 + 2
REPS = 3


def main():
    logs = [int(a) for a in sys.argv[1:]] or [16, 18]
    ctx = Context(0)
    rate = modmul_rate(ctx)
    print("Fq products (lazy 29-bit form, cq_bench_modmul_dev): %.1f G/s" % (rate / 1e9), flush=True)
    print("products per decompressed G2 point: %d (%d of them the root)" % (PRODUCTS_PER_POINT, ROOT_PRODUCTS), flush=True)
    for lg in logs:
        count = 1 << lg
        src = G2Srs.setup_from_toxic_waste(ctx, count, fr_to_mont(0x1234567890ABCDEF1234567))
        raw, proc = src.write(SERDE_RAW_BYTES), src.write(SERDE_PROCESSED)
        pts = src.download()
        src.close()
        line = {}
        for name, data, fmt in (("processed", proc, SERDE_PROCESSED), ("raw_checked", raw, SERDE_RAW_BYTES)):
            wall, kern = [], []
            for rep in range(REPS + 1):  # the first read grows the scratch buffers
                ctx.profile_enable(True)
                ctx.sync()
                t = time.perf_counter()
                p = G2Srs.read(ctx, data, fmt)
                ctx.sync()
                dt = time.perf_counter() - t
                ms, calls = ctx.profile_read(PROF_G2_DECOMPRESS)
                ctx.profile_enable(False)
                if rep:
                    wall.append(dt * 1e3)
                    kern.append(ms)
                    assert calls == (1 if fmt == SERDE_PROCESSED else 0)
                if rep == REPS:
                    assert np.array_equal(p.download(), pts), "the read does not reproduce the SRS"
                p.close()
            line[name] = (min(wall), min(kern))
        host = []
        for rep in range(2):  # the host loop of cq_g2_srs_create(checked = 1): one thread, coordinates and the twist equation
            t = time.perf_counter()
            p = G2Srs(ctx, pts, checked=True)
            ctx.sync()
            host.append((time.perf_counter() - t) * 1e3)
            p.close()
        model_ms = PRODUCTS_PER_POINT * count / rate * 1e3
        wall_p, kern_p = line["processed"]
        print("count=2^%d (%.1f MiB processed / %.1f MiB raw): read processed %.2f ms, read raw checked %.2f ms, "
              "cq_g2_srs_create(checked) from host points %.1f ms; g2_decompress_kernel %.3f ms vs %.3f ms = %d products x %d points / rate: "
              "ratio %.2f" % (lg, len(proc) / 2**20, len(raw) / 2**20, wall_p, line["raw_checked"][0], min(host), kern_p, model_ms,
                              PRODUCTS_PER_POINT, count, kern_p / model_ms), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()

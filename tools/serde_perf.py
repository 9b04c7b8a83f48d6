"""Load-time figures of the serialized SRS: wall time of cq_params_read in SerdeFormat::Processed and in checked RawBytes, the
decompression kernel's own time (HIP events, CQ_PROF_G1_DECOMPRESS), and the chip's Fq product rate from the same run
(cq_bench_modmul_dev, lazy 29-bit form) -- so that the kernel can be held against
    products per point x points / measured product rate.

usage: python tools/serde_perf.py [k ...]      (default: 18 20)
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sha2_on_cq_halo2_amd import Context, ParamsKZG
from sha2_on_cq_halo2_amd.api import PROF_G1_DECOMPRESS, SERDE_PROCESSED, SERDE_RAW_BYTES, fr_to_mont

# csrc/sqrt29.hpp (W = 4) and g1_decompress_kernel: x R', x^2, x^3, the 14 table entries, 4 squarings for each of the 62
# digits below the top one and a product for each non-zero one, y^2 and the reduction of the root check, y out of Montgomery
# form, x and y to the memory form
Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
_DIGITS = [((Q + 1) // 4 >> (4 * j)) & 15 for j in range(63)]
PRODUCTS_PER_POINT = 3 + 14 + 4 * 62 + sum(1 for d in _DIGITS[:62] if d) + 2 + 3
REPS = 3


def modmul_rate(ctx):
    lanes, iters = 256 * 256 * 8, 4096
    buf = ctx.alloc(lanes * 32)
    best = 0.0
    for _ in range(3):  # the first launch warms up
        ctx.sync()
        t = time.perf_counter()
        ctx._chk(ctx.lib.cq_bench_modmul_dev(ctx.h, buf.ptr, lanes, iters, 2))
        ctx.sync()
        best = max(best, lanes * iters / (time.perf_counter() - t))
    buf.free()
    return best


def main():
    ks = [int(a) for a in sys.argv[1:]] or [18, 20]
    ctx = Context(0)
    ctx._chk(ctx.lib.cq_msm_set_precompute(ctx.h, 0))  # the readers' own work, not the window tables both build afterwards
    rate = modmul_rate(ctx)
    print("Fq products (lazy 29-bit form, cq_bench_modmul_dev): %.1f G/s" % (rate / 1e9), flush=True)
    print("products per decompressed point: %d" % PRODUCTS_PER_POINT, flush=True)
    for k in ks:
        n = 1 << k
        src = ParamsKZG.setup_from_toxic_waste(ctx, k, fr_to_mont(0x1234567890ABCDEF1234567))
        raw, proc = src.write_raw(), src.write(SERDE_PROCESSED)
        src.close()
        line = {}
        for name, data, fmt in (("processed", proc, SERDE_PROCESSED), ("raw_checked", raw, SERDE_RAW_BYTES)):
            wall = []
            kern = []
            for rep in range(REPS + 1):  # the first read grows the scratch buffers
                ctx.profile_enable(True)
                ctx.sync()
                t = time.perf_counter()
                p = ParamsKZG.read(ctx, data, fmt)
                ctx.sync()
                dt = time.perf_counter() - t
                ms, calls = ctx.profile_read(PROF_G1_DECOMPRESS)
                ctx.profile_enable(False)
                if rep:
                    wall.append(dt * 1e3)
                    kern.append(ms)
                    assert calls == (2 if fmt == SERDE_PROCESSED else 0)
                if rep == REPS and fmt == SERDE_PROCESSED:
                    assert p.write_raw() == raw, "Processed read does not reproduce the raw SRS"
                p.close()
            line[name] = (min(wall), min(kern))
        points = 2 * n
        model_ms = PRODUCTS_PER_POINT * points / rate * 1e3
        wall_p, kern_p = line["processed"]
        print("k=%d (%d points, %.1f MiB processed / %.1f MiB raw): read processed %.2f ms, read raw checked %.2f ms; "
              "g1_decompress_kernel %.3f ms (2 launches) vs %.3f ms = %d products x %d points / rate: ratio %.2f"
              % (k, points, len(proc) / 2**20, len(raw) / 2**20, wall_p, line["raw_checked"][0], kern_p, model_ms,
                 PRODUCTS_PER_POINT, points, kern_p / model_ms), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()

"""g_to_lagrange over 2^k powers [s^i]_1 on the GPU by one of the two G1 FFTs: `old` = cq_g_to_lagrange_dev (double-and-add
twiddle products), `new` = cq_g_to_lagrange_windowed_dev (fixed-window chain, csrc/g1window.hpp).  One path and one size per
process: a warm-up run of the same shape, then `--reps` timed runs (host clock around a call that ends in a stream
synchronise), every time and the best printed, and a digest of the output so that the two paths can be compared.
    python tools/g1fft_perf.py --k 16 --path new"""
import argparse, hashlib, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sha2_on_cq_halo2_amd import Context
from sha2_on_cq_halo2_amd.sha_circuit import srs_powers_dev

ap = argparse.ArgumentParser()
ap.add_argument("--k", type=int, required=True)
ap.add_argument("--path", choices=["old", "new"], required=True)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
ctx = Context(0)
n = 1 << a.k
g = srs_powers_dev(ctx, 0x1234567890ABCDEF1234567, n)
out = ctx.alloc(n * 64)
fn = ctx.lib.cq_g_to_lagrange_dev if a.path == "old" else ctx.lib.cq_g_to_lagrange_windowed_dev
times = []
for rep in range(a.reps + 1):  # rep 0: warm-up
    ctx.sync()
    t = time.perf_counter()
    ctx._chk(fn(ctx.h, g.ptr, a.k, out.ptr))
    ctx.sync()
    times.append((time.perf_counter() - t) * 1e3)
digest = hashlib.sha256(out.download((n, 8)).tobytes()).hexdigest()[:16]
print("g_to_lagrange k=%d path=%s warmup %.2f ms, runs %s ms, best %.2f ms, sha256 %s"
      % (a.k, a.path, times[0], " ".join("%.2f" % t for t in times[1:]), min(times[1:]), digest), flush=True)
ctx.close()

"""Stand-alone timing of cq_batch_invert_assigned_dev (poly.hip: the resolve of Assigned columns) at the shape a k = 18
proof with 8 advice columns hands over, for rational-cell shares of 1/64, 1/8 and all of the usable rows, next to the
yardstick: cq_batch_invert_dev over a dense array of the same element count.  Nothing else on the GPU.
   python3 tools/assigned_perf.py [k] [columns] [reps]
Every figure is one call plus the wait for it (wall clock, median and minimum of `reps` runs after 5 warm-up calls); the
resolve calls include what the entry point does around the kernels (gathering the lists, their check, the verdict read).
profiles/r13_assigned_resolve.txt is the run that chose the fused kernel over the two-step form it was measured against."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sha2_on_cq_halo2_amd import Context

k = int(sys.argv[1]) if len(sys.argv) > 1 else 18
ncols = int(sys.argv[2]) if len(sys.argv) > 2 else 8
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 30
n = 1 << k
usable = n - 6
ctx = Context(0)
rs = np.random.RandomState(13)


def elements(count):
    a = rs.randint(0, 2**63, size=(count, 4), dtype=np.int64).astype(np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)
    return a


def timed(call):
    for _ in range(5):
        call()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t) * 1e6)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


print("resolve of %d Assigned columns of 2^%d cells (%d usable rows), %d runs each; us, median (min)" % (ncols, k, usable, reps))
print("%-8s %10s  %-22s %s" % ("share", "cells", "batch_invert_dev", "batch_invert_assigned_dev"))
for share in (64, 8, 1):
    per_col = usable // share
    nums = [ctx.to_device(elements(n)) for _ in range(ncols)]
    rows = [ctx.to_device(np.sort(rs.choice(usable, per_col, replace=False)).astype(np.uint32)) for _ in range(ncols)]
    dens = [ctx.to_device(elements(per_col)) for _ in range(ncols)]
    descr = [(nums[c].ptr, rows[c].ptr, dens[c].ptr, per_col) for c in range(ncols)]
    outs = [b.ptr for b in nums]  # in place, as create_proof resolves
    total = per_col * ncols
    dense = ctx.to_device(elements(total))

    def yardstick():
        ctx._chk(ctx.lib.cq_batch_invert_dev(ctx.h, dense.ptr, total))
        ctx.sync()

    print("%-8s %10d  %-22s %s" % ("1/%d" % share, total, "%.1f (%.1f)" % timed(yardstick),
                                   "%.1f (%.1f)" % timed(lambda: ctx.batch_invert_assigned_dev(descr, n, outs))), flush=True)
    for b in nums + rows + dens + [dense]:
        b.free()

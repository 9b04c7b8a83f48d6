"""G2 timings on one GPU: best_multiexp over G2 at 2^16 / 2^18 / 2^20 terms, the G2 SRS generation rate
(cq_g2_srs_setup_from_toxic_waste) and StaticTableValues::commit of the 2^16 spread table.  Wall times of the C calls
(each returns after its stream has drained), best of --reps after one warm-up.
   python3 tools/g2_perf.py [--reps 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sha2_on_cq_halo2_amd import Context, G2Srs, StaticTable  # noqa: E402
from sha2_on_cq_halo2_amd.api import fr_to_mont  # noqa: E402
from sha2_on_cq_halo2_amd.sha_circuit import small_to_mont, spread16  # noqa: E402


def best(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    ctx = Context(0)
    s = np.ascontiguousarray(fr_to_mont(0x1D2C3B4A59687706F5E4D3C2B1A09F8E7D6C5B4A39281706F5E4D3C2B1A0918)).reshape(4)
    rows = []
    count = (1 << 20) + 1
    t = best(lambda: G2Srs.setup_from_toxic_waste(ctx, count, s).close(), a.reps)
    rows.append({"what": "g2_srs_setup", "points": count, "ms": round(t * 1e3, 2), "Mpoints_per_s": round(count / t / 1e6, 3)})
    srs = G2Srs.setup_from_toxic_waste(ctx, count, s)
    rs = np.random.RandomState(1)
    for lg in (16, 18, 20):
        n = 1 << lg
        sc = rs.randint(0, 2**63, size=(n, 4), dtype=np.int64).astype(np.uint64)
        sc[:, 3] &= np.uint64((1 << 60) - 1)
        d = ctx.to_device(sc)
        t = best(lambda: ctx.best_multiexp_g2_dev(d, srs.dev, n), a.reps)
        rows.append({"what": "g2_msm", "log_n": lg, "ms": round(t * 1e3, 2), "Mscalars_per_s": round(n / t / 1e6, 2)})
        d.free()
    idx = np.arange(1 << 16, dtype=np.uint64)
    tab = StaticTable.setup_from_toxic_waste(ctx, small_to_mont(spread16(idx)), s)
    t = best(lambda: tab.commit(srs, 1 << 16, 1 << 16), a.reps)
    rows.append({"what": "static_table_commit", "table": "spread", "log_N": 16, "ms": round(t * 1e3, 2)})
    for r in rows:
        print(json.dumps(r))
    tab.close()
    srs.close()
    ctx.close()


if __name__ == "__main__":
    main()

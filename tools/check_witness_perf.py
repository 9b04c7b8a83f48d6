"""Median time of one `ProvingKey.check_witness` next to the median time of one proof of the same key and witness, in
one process: ShaPlonkWorkload at k = 16 / 18 / 20 and ShaCqWorkload at k = 18, advice on the device and on the host.

Both calls end in a stream synchronise inside the library, so a host clock around them measures the whole thing.

    python tools/check_witness_perf.py [--sizes plonk:16,plonk:18,plonk:20,cq:18] [--reps 15] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="plonk:16,plonk:18,plonk:20,cq:18")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from sha2_on_cq_halo2_amd import Context
    from sha2_on_cq_halo2_amd.sha_circuit import ShaCqWorkload, ShaPlonkWorkload

    ctx = Context(0)
    for item in args.sizes.split(","):
        kind, k = item.split(":")
        k = int(k)
        wl = (ShaPlonkWorkload if kind == "plonk" else ShaCqWorkload)(ctx, k)
        ptrs = [c.ptr for c in wl.cols]
        host = [c.download((wl.n, 4)) for c in wl.cols]
        assert wl.pk.check_witness(ptrs) == (0, []) and wl.pk.check_witness(host) == (0, [])
        seed = [0]

        def prove():
            seed[0] += 1
            wl.prove(seed=seed[0])

        def prove_host():
            seed[0] += 1
            wl.pk.create_proof(host, seed=seed[0])

        row = {"workload": "Sha%sWorkload" % ("Plonk" if kind == "plonk" else "Cq"), "k": k, "advice_columns": len(ptrs)}
        for name, fn in (("check_dev_ms", lambda: wl.pk.check_witness(ptrs, max_failures=0)),
                         ("check_host_ms", lambda: wl.pk.check_witness(host, max_failures=0)),
                         ("proof_dev_ms", prove), ("proof_host_ms", prove_host)):
            med, lo, hi = median_ms(fn, args.reps, args.warmup)
            row[name] = round(med, 3)
            row[name + "_range"] = [round(lo, 3), round(hi, 3)]
        print(json.dumps(row), flush=True)
        wl.close()
    ctx.close()


if __name__ == "__main__":
    main()

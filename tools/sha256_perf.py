"""Median time of `Sha256Circuit.synthesize` (the host compression chain, the upload of its words, the expansion kernel
and the wait for it), of the witness check and of one proof, at k = 14 and k = 18 with the largest block count each
holds; next to them the proof of `ShaPlonkWorkload` at the same k, in the same process, for scale.

Every timed call ends in a stream synchronise (synthesize: an explicit one here), so a host clock around it measures
the whole thing.

    python tools/sha256_perf.py [--sizes 14,18] [--reps 15] [--warmup 3]
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
    return round(statistics.median(ts), 3), [round(min(ts), 3), round(max(ts), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="14,18")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert args.reps >= 10, "a median of at least 10 runs"
    import hashlib

    from sha2_on_cq_halo2_amd import Context
    from sha2_on_cq_halo2_amd.api import Sha256Circuit
    from sha2_on_cq_halo2_amd.sha_circuit import ShaPlonkWorkload

    ctx = Context(0)
    for k in (int(s) for s in args.sizes.split(",")):
        t0 = time.perf_counter()
        c = Sha256Circuit(ctx, k)
        keygen_s = time.perf_counter() - t0
        msg = bytes(i % 251 for i in range(64 * c.blocks - 9))
        assert c.check(msg) == (0, []) and c.digest == hashlib.sha256(msg).digest()
        ptrs, seed = [b.ptr for b in c.cols], [0]

        def synthesize():
            c.synthesize(msg)
            ctx.sync()

        def prove():
            seed[0] += 1
            c.pk.create_proof_dev(ptrs, seed=seed[0], instances=c.instances)

        row = {"circuit": "Sha256Circuit", "k": k, "blocks": c.blocks, "message_bytes": len(msg), "advice_columns": len(ptrs),
               "degree": c.cs.degree(), "proof_bytes": c.pk.proof_size, "keygen_s": round(keygen_s, 2)}
        for name, fn in (("synthesize_ms", synthesize), ("check_ms", lambda: c.pk.check_witness(ptrs, instances=c.instances, max_failures=0)),
                         ("proof_ms", prove)):
            row[name], row[name + "_range"] = median_ms(fn, args.reps, args.warmup)
        c.close()
        wl = ShaPlonkWorkload(ctx, k)
        row["sha_plonk_workload_proof_ms"], row["sha_plonk_workload_proof_ms_range"] = median_ms(lambda: wl.prove(seed=3), args.reps, args.warmup)
        wl.close()
        print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()

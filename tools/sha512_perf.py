"""Median time of `Sha512Circuit.synthesize` (the upload of the message words, the chain kernel, the expansion kernel, the
digest's download and the wait for it), of the witness check and of one proof, at k = 14 and k = 18 with the largest
block count each holds; next to them `Sha256Circuit` at the same k with the largest block count it holds, in the same
process, as the yardstick.  A SHA-512 block is 128 message bytes, a SHA-256 block 64: `message_bytes` says what each
circuit hashes in its rows.

Every timed call ends in a stream synchronise (Sha256Circuit.synthesize: an explicit one here), so a host clock around it
measures the whole thing.

    python tools/sha512_perf.py [--sizes 14,18] [--reps 15] [--warmup 3]
"""
import argparse
import hashlib
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


def circuit_row(ctx, name, make, block_bytes, tail_bytes, digest_of, reps, warmup):
    t0 = time.perf_counter()
    c = make()
    keygen_s = time.perf_counter() - t0
    msg = bytes(i % 251 for i in range(block_bytes * c.blocks - tail_bytes))
    assert c.check(msg) == (0, []) and c.digest == digest_of(msg).digest()
    ptrs, seed = [b.ptr for b in c.cols], [0]

    def synthesize():
        c.synthesize(msg)
        ctx.sync()

    def prove():
        seed[0] += 1
        c.pk.create_proof_dev(ptrs, seed=seed[0], instances=c.instances)

    row = {"circuit": name, "k": c.k, "blocks": c.blocks, "message_bytes": len(msg), "rows": c.rows, "advice_columns": len(ptrs),
           "degree": c.cs.degree(), "advice_queries": len(c.cs.advice_queries), "proof_bytes": c.pk.proof_size, "keygen_s": round(keygen_s, 2)}
    for leg, fn in (("synthesize_ms", synthesize), ("check_ms", lambda: c.pk.check_witness(ptrs, instances=c.instances, max_failures=0)),
                    ("proof_ms", prove)):
        row[leg], row[leg + "_range"] = median_ms(fn, reps, warmup)
    c.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="14,18")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert args.reps >= 10, "a median of at least 10 runs"

    from sha2_on_cq_halo2_amd import Context
    from sha2_on_cq_halo2_amd.api import Sha256Circuit, Sha512Circuit

    ctx = Context(0)
    for k in (int(s) for s in args.sizes.split(",") if s):
        wide = circuit_row(ctx, "Sha512Circuit", lambda: Sha512Circuit(ctx, k), 128, 17, hashlib.sha512, args.reps, args.warmup)
        print(json.dumps(wide), flush=True)
        narrow = circuit_row(ctx, "Sha256Circuit", lambda: Sha256Circuit(ctx, k), 64, 9, hashlib.sha256, args.reps, args.warmup)
        print(json.dumps(narrow), flush=True)
        print(json.dumps({"k": k, **{leg + "_sha512_over_sha256": round(wide[leg + "_ms"] / narrow[leg + "_ms"], 3)
                                     for leg in ("synthesize", "check", "proof")},
                          "message_bytes_sha512_over_sha256": round(wide["message_bytes"] / narrow["message_bytes"], 3)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()

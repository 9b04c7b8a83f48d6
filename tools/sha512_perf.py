"""Median time of `Sha512Circuit.synthesize` (the upload of the message words, the chain kernel, the expansion kernel, the
digest's download and the wait for it), of the witness check and of one proof, at k = 14 and k = 18 with the largest
block count each holds; next to them `Sha256Circuit` at the same k with the largest block count it holds, in the same
process, as the yardstick.  A SHA-512 block is 128 message bytes, a SHA-256 block 64: `message_bytes` says what each
circuit hashes in its rows.

Every timed call ends in a stream synchronise (Sha256Circuit.synthesize: an explicit one here), so a host clock around it
measures the whole thing.

Two more legs measure the wired segments (sha512_segments.py) at --segments-k (18): `batch`, the largest batch of one-block
messages that fits, synthesised through cq_sha512_synthesize_dev (Sha512BatchCircuit, the yardstick) and through
cq_sha512_synthesize_segments_dev (the `batch` plan: the whole `synthesize`, and the entry point alone on the word buffer as
it is on the device); and `merkle`, the deepest Merkle tree over 64-byte leaves that fits: the entry point with a stream
synchronise, then the witness check and one proof.

The `hmac` leg (not run by default) is as many independent HMAC-SHA-512 (64-byte key, one message block) as 2^segments-k
rows hold in one plan: cq_sha512_synthesize_xors_dev plus a stream synchronise, the same plan with the Xor words as Private
words through cq_sha512_synthesize_segments_dev -- the difference is what the XOR units cost -- then `synthesize`, the witness
check and one proof of the keyed circuit.

    python tools/sha512_perf.py [--sizes 14,18] [--legs circuits,batch,merkle[,hmac]] [--segments-k 18] [--reps 15] [--warmup 3]
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


def segment_legs(ctx, c, inputs, reps, warmup):
    """The entry point alone (queued, then a stream synchronise), the witness check and one proof of a Sha512SegmentsCircuit
    whose word buffer `synthesize(*inputs)` has uploaded."""
    import ctypes as C

    assert c.check(*inputs) == (0, [])
    ptrs, seed = [b.ptr for b in c.cols], [0]
    arr = (C.c_void_p * len(ptrs))(*ptrs)

    def entry():
        c._call(arr)
        ctx.sync()

    def prove():
        seed[0] += 1
        c.pk.create_proof_dev(ptrs, seed=seed[0], instances=c.instances)

    row = {}
    for leg, fn in (("entry_ms", entry), ("check_ms", lambda: c.pk.check_witness(ptrs, instances=c.instances, max_failures=0)), ("proof_ms", prove)):
        row[leg], row[leg + "_range"] = median_ms(fn, reps, warmup)
    return row


def batch_rows(ctx, k, reps, warmup):
    """The largest batch of one-block messages at 2^k rows, through both entry points."""
    from sha2_on_cq_halo2_amd import sha512_circuit as SC
    from sha2_on_cq_halo2_amd import sha512_segments as SS
    from sha2_on_cq_halo2_amd.api import Sha512BatchCircuit, Sha512SegmentsCircuit

    count = SC.usable_rows(k) // SC.rows_for(1)
    msgs = [bytes((i + 3 * j) % 251 for i in range(j % 112)) for j in range(count)]
    digests = [hashlib.sha512(m).digest() for m in msgs]
    old = Sha512BatchCircuit(ctx, k, [1] * count)
    assert old.check(msgs) == (0, []) and old.digests == digests
    row = {"leg": "batch", "entry_point": "cq_sha512_synthesize_dev", "k": k, "messages": count, "rows": old.rows}
    row["synthesize_ms"], row["synthesize_ms_range"] = median_ms(lambda: old.synthesize(msgs), reps, warmup)  # ends in the digests' download
    old.close()
    print(json.dumps(row), flush=True)
    new = Sha512SegmentsCircuit(ctx, k, SS.batch([1] * count))
    values = [SC.pad(m, 1) for m in msgs]
    new.synthesize(values)
    assert new.digests == digests
    wired = {"leg": "batch", "entry_point": "cq_sha512_synthesize_segments_dev", "k": k, "messages": count, "rows": new.rows, "levels": 1}
    wired["synthesize_ms"], wired["synthesize_ms_range"] = median_ms(lambda: new.synthesize(values), reps, warmup)  # upload, entry, download
    wired.update(segment_legs(ctx, new, (values,), reps, warmup))
    new.close()
    print(json.dumps(wired), flush=True)
    print(json.dumps({"leg": "batch", "k": k, "synthesize_segments_over_plain": round(wired["synthesize_ms"] / row["synthesize_ms"], 3)}), flush=True)


def merkle_row(ctx, k, reps, warmup):
    """The deepest Merkle tree over 64-byte leaves at 2^k rows."""
    from sha2_on_cq_halo2_amd import sha512_circuit as SC
    from sha2_on_cq_halo2_amd.api import Sha512MerkleCircuit

    depth = 1
    while ((2 << depth) - 1) * SC.rows_for(2) <= SC.usable_rows(k):
        depth += 1
    c = Sha512MerkleCircuit(ctx, k, depth)
    level = leaves = [bytes((i + 5 * j) % 251 for i in range(64)) for j in range(1 << depth)]
    while len(level) > 1:
        level = [hashlib.sha512(level[i] + level[i + 1]).digest() for i in range(0, len(level), 2)]
    c.synthesize(leaves)
    assert c.digests == level
    row = {"leg": "merkle", "k": k, "depth": depth, "leaves": len(leaves), "segments": len(c.plan.segments), "levels": depth, "rows": c.rows,
           "proof_bytes": c.pk.proof_size}
    row.update(segment_legs(ctx, c, (leaves,), reps, warmup))
    c.close()
    print(json.dumps(row), flush=True)


def hmac_row(ctx, k, reps, warmup):
    """The largest count of independent HMAC-SHA-512 (64-byte key, 104-byte message: one message block) at 2^k rows."""
    import ctypes as C
    import hmac

    import numpy as np

    from sha2_on_cq_halo2_amd import sha512_circuit as SC
    from sha2_on_cq_halo2_amd import sha512_segments as SS
    from sha2_on_cq_halo2_amd import sha512_xor as SX

    key_bytes, message_bytes = 64, 104
    one = SX.hmac_sha512(key_bytes, message_bytes)
    count, nvars = SC.usable_rows(k) // SX.rows_for(one), key_bytes // 8

    def moved(s, i, strip):  # HMAC i of the plan: its own vars and segments; `strip`: the Xor words as Private words
        if isinstance(s, SX.Xor):
            return SS.PRIVATE if strip else SX.Xor(moved(s.x, i, strip), moved(s.y, i, strip))
        if isinstance(s, SS.Var):
            return SS.Var(s.index + nvars * i)
        return SS.DigestWord(s.segment + 2 * i, s.word) if isinstance(s, SS.DigestWord) else s

    def repeated(strip):
        segs = tuple(SS.Segment(seg.blocks, tuple(moved(s, i, strip) for s in seg.sources)) for i in range(count) for seg in one.segments)
        return SS.Plan(segs, tuple((2 * i + 1, 8) for i in range(count)))

    keys = [hashlib.sha512(b"key %d" % i).digest() for i in range(count)]
    messages = [bytes((i + 3 * j) % 256 for j in range(message_bytes)) for i in range(count)]
    tags = [hmac.new(key, m, "sha512").digest() for key, m in zip(keys, messages)]
    words = lambda data: [int(x) for x in np.frombuffer(data, dtype=">u8")]
    n = 1 << k
    cols = [ctx.alloc(32 * n) for _ in range(SC.ADVICE_COLUMNS)]
    arr = (C.c_void_p * len(cols))(*[b.ptr for b in cols])
    row = {"leg": "hmac", "hmac": "independent HMAC-SHA-512, 64-byte key, 104-byte message", "k": k, "hmacs": count, "segments": 2 * count,
           "blocks": 4 * count, "xor_units": 2 * nvars * count, "rows": count * SX.rows_for(one)}
    legs, bufs = [], []
    for strip in (False, True):
        plan = repeated(strip)
        low = SX.lower(plan)
        if strip:  # the key block's words are private words, in word order before the message's
            values = [x for i in range(count) for x in ([w ^ SX.HMAC_IPAD for w in words(keys[i])] + words(messages[i]), [w ^ SX.HMAC_OPAD for w in words(keys[i])])]
            buf = SS.word_buffer(low, values)
        else:
            buf = SS.word_buffer(low, [x for i in range(count) for x in (words(messages[i]), [])], [w for key in keys for w in words(key)])
        words_dev, digests_dev = ctx.to_device(buf), ctx.alloc(64 * len(low.seg_blocks) + 8 * len(low.xors))
        bufs += [words_dev, digests_dev]

        def call(low=low, words_dev=words_dev, digests_dev=digests_dev, strip=strip):
            head = (ctx.h, 12, low.seg_blocks.ctypes.data, len(low.seg_blocks), low.seg_variant.ctypes.data, low.sources.ctypes.data, None)
            tail = (words_dev.ptr, low.words_len, n, arr, digests_dev.ptr)
            if strip:
                ctx._chk(ctx.lib.cq_sha512_synthesize_segments_dev(*head, *tail))
            else:
                ctx._chk(ctx.lib.cq_sha512_synthesize_xors_dev(*head, low.xors.ctypes.data, len(low.xors), *tail))
            ctx.sync()

        call()
        got = digests_dev.download((2 * count, 8), np.uint64)[1::2].astype(">u8")
        assert [t.tobytes() for t in got] == tags
        legs.append(("segments_dev_private_key_blocks_ms" if strip else "xors_dev_ms", call))
    for name, fn in legs + [("xors_dev_again_ms", legs[0][1])]:
        row[name], row[name + "_range"] = median_ms(fn, reps, warmup)
    for b in cols + bufs:
        b.close()
    t0 = time.perf_counter()
    c = SX.Sha512XorSegmentsCircuit(ctx, k, repeated(False))
    row["keygen_s"] = round(time.perf_counter() - t0, 2)
    values, shared = [x for i in range(count) for x in (words(messages[i]), [])], [w for key in keys for w in words(key)]
    assert c.check(values, shared) == (0, []) and c.digests == tags
    ptrs, seed = [b.ptr for b in c.cols], [0]

    def prove():
        seed[0] += 1
        c.pk.create_proof_dev(ptrs, seed=seed[0], instances=c.instances)

    def synthesize():
        c.synthesize(values, shared)
        ctx.sync()

    for name, fn in (("synthesize_ms", synthesize), ("check_ms", lambda: c.pk.check_witness(ptrs, instances=c.instances, max_failures=0)),
                     ("proof_ms", prove)):
        row[name], row[name + "_range"] = median_ms(fn, reps, warmup)
    row["proof_bytes"] = c.pk.proof_size
    c.close()
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="14,18")
    ap.add_argument("--legs", default="circuits,batch,merkle")
    ap.add_argument("--segments-k", type=int, default=18)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert args.reps >= 10, "a median of at least 10 runs"

    from sha2_on_cq_halo2_amd import Context
    from sha2_on_cq_halo2_amd.api import Sha256Circuit, Sha512Circuit

    ctx = Context(0)
    legs = args.legs.split(",")
    for k in (int(s) for s in args.sizes.split(",") if s and "circuits" in legs):
        wide = circuit_row(ctx, "Sha512Circuit", lambda: Sha512Circuit(ctx, k), 128, 17, hashlib.sha512, args.reps, args.warmup)
        print(json.dumps(wide), flush=True)
        narrow = circuit_row(ctx, "Sha256Circuit", lambda: Sha256Circuit(ctx, k), 64, 9, hashlib.sha256, args.reps, args.warmup)
        print(json.dumps(narrow), flush=True)
        print(json.dumps({"k": k, **{leg + "_sha512_over_sha256": round(wide[leg + "_ms"] / narrow[leg + "_ms"], 3)
                                     for leg in ("synthesize", "check", "proof")},
                          "message_bytes_sha512_over_sha256": round(wide["message_bytes"] / narrow["message_bytes"], 3)}), flush=True)
    if "batch" in legs:
        batch_rows(ctx, args.segments_k, args.reps, args.warmup)
    if "merkle" in legs:
        merkle_row(ctx, args.segments_k, args.reps, args.warmup)
    if "hmac" in legs:
        hmac_row(ctx, args.segments_k, args.reps, args.warmup)
    ctx.close()


if __name__ == "__main__":
    main()

"""Median time of `Sha256Circuit.synthesize` (the host compression chain, the upload of its words, the expansion kernel
and the wait for it), of the witness check and of one proof, at k = 14 and k = 18 with the largest block count each
holds; next to them the proof of `ShaPlonkWorkload` at the same k, in the same process, for scale.

Every timed call ends in a stream synchronise (synthesize: an explicit one here), so a host clock around it measures
the whole thing.

With --segments-k K (0 = off): the wired-segment circuits at 2^K rows -- `Sha256BatchCircuit` of as many one-block
messages as fit and `Sha256MerkleCircuit` of the largest depth that fits: synthesize (word upload, the entry point with
its device compression chains, digest download), check and proof; beside the batch, `Sha256Circuit.synthesize` (the host
compression chain) at the same total block count.  Then a sweep over the segment count at 2^K rows, entry point against
entry point with no key: cq_sha256_synthesize_segments_dev on c one-block segments whose words are already on the
device, and cq_sha256_synthesize_dev on one message of c blocks, each followed by a stream synchronise.

With --path-k K (0 = off): `Sha256MerklePathCircuit` of depth 32 with as many paths as 2^K rows hold, next to a plan of
the same shape without choices -- per path a chain of 32 two-block segments, each wired to the one below by DigestWord
alone -- through cq_sha256_synthesize_segments_dev: entry point + synchronise, the wrapper's synthesize, check and proof of
both.  The difference of the two entry-point times is the choice fetch of the chain kernel plus the fill launch.

With --varlen-k K (0 = off): `Sha256VarCircuit` over segments of 1, 2, 4, 8 blocks in turn, as many as 2^K rows hold, with
messages of mixed lengths (raw bytes in, padded on the device), next to `Sha256BatchCircuit` at the same block counts, whose
messages fill their segments: the wrapper's synthesize, the entry point + synchronise, check and proof of both.

With --states-k K (0 = off): as many one-block segments as 2^K rows hold, no key, words on the device: the entry point + a
synchronise through cq_sha256_synthesize_segments_dev, through cq_sha256_synthesize_states_dev with init_sources = NULL,
with all-IV initial sources, and with every segment's state eight Private words of the buffer.

With --stream-k K (0 = off): a 1 MiB message through `Sha256Stream` with bodies and a tail of as many blocks as 2^K rows
hold: the whole `prove` (one median over --reps runs would take minutes: 3 runs), per proof and in total, next to
`Sha256Circuit`'s proof at the same K.

With --hmac-k K (0 = off): as many independent HMAC-SHA-256 (32-byte key, one message block) as 2^K rows hold in one plan
with XOR-wired key blocks: cq_sha256_synthesize_xors_dev + synchronise with no key, beside the same plan with the Xor words
as Private words through cq_sha256_synthesize_states_dev; then the wrapper's synthesize, check and proof.

    python tools/sha256_perf.py [--sizes 14,18] [--segments-k 18] [--path-k 18] [--varlen-k 18] [--states-k 18] [--stream-k 18] [--hmac-k 18]
                                [--sweep 1,2,4,...] [--reps 15] [--warmup 3]
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


def timed(row, legs, reps, warmup):
    for name, fn in legs:
        row[name], row[name + "_range"] = median_ms(fn, reps, warmup)


def segment_legs(ctx, k, sweep, reps, warmup):
    import ctypes as C
    import hashlib

    import numpy as np

    from sha2_on_cq_halo2_amd import sha256_circuit as SC
    from sha2_on_cq_halo2_amd.api import Sha256BatchCircuit, Sha256Circuit, Sha256MerkleCircuit

    usable = SC.usable_rows(k)
    count = usable // SC.rows_for(1)
    depth = (usable // SC.rows_for(2) + 1).bit_length() - 1  # 2^depth - 1 two-block nodes
    messages = [bytes((i + j) % 251 for i in range(55 - j % 7)) for j in range(count)]
    leaves = [hashlib.sha256(bytes([i % 256, i // 256])).digest() for i in range(1 << depth)]
    for name, make, arg, shape in (("Sha256BatchCircuit", lambda: Sha256BatchCircuit(ctx, k, [1] * count), messages, {"segments": count, "blocks": count, "levels": 1}),
                                   ("Sha256MerkleCircuit", lambda: Sha256MerkleCircuit(ctx, k, depth), leaves,
                                    {"depth": depth, "segments": (1 << depth) - 1, "blocks": 2 * ((1 << depth) - 1), "levels": depth})):
        t0 = time.perf_counter()
        c = make()
        row = {"circuit": name, "k": k, **shape, "rows": c.rows, "keygen_s": round(time.perf_counter() - t0, 2)}
        assert c.check(arg) == (0, [])
        ptrs, seed = [b.ptr for b in c.cols], [0]
        arr = (C.c_void_p * len(ptrs))(*ptrs)

        def call():  # the entry point alone: the word buffer of the last synthesize is still on the device
            ctx._chk(ctx.lib.cq_sha256_synthesize_segments_dev(ctx.h, c.table_bits, c._seg_blocks.ctypes.data, len(c._seg_blocks), c._sources.ctypes.data,
                                                               c._words.ptr, c._words_len, c.n, arr, c._digests.ptr))
            ctx.sync()

        def prove():
            seed[0] += 1
            c.pk.create_proof_dev(ptrs, seed=seed[0], instances=c.instances)

        timed(row, (("synthesize_ms", lambda: c.synthesize(arg)), ("synthesize_call_ms", call),
                    ("check_ms", lambda: c.pk.check_witness(ptrs, instances=c.instances, max_failures=0)), ("proof_ms", prove)), reps, warmup)
        c.close()
        if name == "Sha256BatchCircuit":  # the host-chain path at the same total block count, same process
            one = Sha256Circuit(ctx, k, count)
            msg = bytes(i % 251 for i in range(64 * count - 9))

            def host():
                one.synthesize(msg)
                ctx.sync()

            timed(row, (("sha256circuit_same_blocks_synthesize_ms", host),), reps, warmup)
            row["synthesize_vs_host_chain"] = round(row["synthesize_ms"] / row["sha256circuit_same_blocks_synthesize_ms"], 3)
            row["synthesize_call_vs_host_chain"] = round(row["synthesize_call_ms"] / row["sha256circuit_same_blocks_synthesize_ms"], 3)
            one.close()
        print(json.dumps(row), flush=True)
    # the sweep: no key, one set of columns
    n = 1 << k
    cols = [ctx.alloc(32 * n) for _ in range(SC.ADVICE_COLUMNS)]
    arr = (C.c_void_p * len(cols))(*[b.ptr for b in cols])
    words = np.array(SC.pad(bytes(i % 251 for i in range(64 * count - 9))), dtype=np.uint32)
    words_dev, digests_dev, digest = ctx.to_device(words), ctx.alloc(32 * count), (C.c_uint32 * 8)()
    for c_ in (int(x) for x in sweep.split(",")):
        c_ = min(c_, count)
        blocks, sources = np.ones(c_, dtype=np.uint32), np.arange(16 * c_, dtype=np.uint32)

        def device():
            ctx._chk(ctx.lib.cq_sha256_synthesize_segments_dev(ctx.h, 12, blocks.ctypes.data, c_, sources.ctypes.data, words_dev.ptr, len(words), n, arr,
                                                               digests_dev.ptr))
            ctx.sync()

        def host():
            ctx._chk(ctx.lib.cq_sha256_synthesize_dev(ctx.h, 12, words.ctypes.data, c_, n, arr, digest))
            ctx.sync()

        row = {"sweep": "one-block segments (device chains) vs one message of as many blocks (host chain)", "k": k, "count": c_}
        timed(row, (("segments_call_ms", device), ("host_chain_call_ms", host)), reps, warmup)
        row["ratio"] = round(row["segments_call_ms"] / row["host_chain_call_ms"], 3)
        print(json.dumps(row), flush=True)
    for b in cols + [words_dev, digests_dev]:
        b.close()


def path_legs(ctx, k, reps, warmup, depth=32):
    import ctypes as C
    import hashlib
    import struct

    from sha2_on_cq_halo2_amd import sha256_circuit as SC
    from sha2_on_cq_halo2_amd import sha256_segments as SS
    from sha2_on_cq_halo2_amd.api import Sha256MerklePathCircuit, Sha256SegmentsCircuit

    paths = SC.usable_rows(k) // (depth * SC.rows_for(2))
    assert paths >= 1, f"2^{k} rows hold no path of depth {depth}"
    node = lambda *key: hashlib.sha256(bytes(key)).digest()
    items = [(node(p), (0x9E3779B9 * (p + 1)) % (1 << depth), [node(p, level) for level in range(depth)]) for p in range(paths)]
    # the same shape without a choice: the left half wired to the segment below, the right half private
    upper = tuple(SS.DigestWord(0, t) for t in range(8)) + (SS.PRIVATE,) * 8
    segs = []
    for p in range(paths):
        for level in range(depth):
            words = tuple(w._replace(segment=len(segs) - 1) if isinstance(w, SS.DigestWord) else w for w in upper) if level else (SS.PRIVATE,) * 16
            segs.append(SS.Segment(2, words + SS.PAD_64_BYTES))
    wired = SS.Plan(tuple(segs), tuple(depth * (p + 1) - 1 for p in range(paths)))
    words_of = lambda data: list(struct.unpack(f">{len(data) // 4}I", data))
    wired_values = [w for leaf, _, siblings in items for w in [words_of(leaf + siblings[0])] + [words_of(s) for s in siblings[1:]]]
    rows = []
    for name, make, arg in (("Sha256MerklePathCircuit", lambda: Sha256MerklePathCircuit(ctx, k, depth, paths), items),
                            ("DigestWord chains, same shape, no choice", lambda: Sha256SegmentsCircuit(ctx, k, wired), wired_values)):
        t0 = time.perf_counter()
        c = make()
        row = {"circuit": name, "k": k, "depth": depth, "paths": paths, "segments": len(c.plan.segments), "levels": depth, "rows": c.rows,
               "choices": len(c._choices), "keygen_s": round(time.perf_counter() - t0, 2)}
        assert c.check(arg) == (0, [])
        ptrs, seed = [b.ptr for b in c.cols], [0]
        arr = (C.c_void_p * len(ptrs))(*ptrs)

        def call():  # the entry point alone: the word buffer of the last synthesize is still on the device
            c._call(arr)
            ctx.sync()

        def prove():
            seed[0] += 1
            c.pk.create_proof_dev(ptrs, seed=seed[0], instances=c.instances)

        timed(row, (("synthesize_ms", lambda: c.synthesize(arg)), ("synthesize_call_ms", call),
                    ("check_ms", lambda: c.pk.check_witness(ptrs, instances=c.instances, max_failures=0)), ("proof_ms", prove)), reps, warmup)
        c.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps({"choice_cost": "entry point + sync, with choices minus without", "k": k,
                      "synthesize_call_ms_difference": round(rows[0]["synthesize_call_ms"] - rows[1]["synthesize_call_ms"], 3),
                      "proof_ms_difference": round(rows[0]["proof_ms"] - rows[1]["proof_ms"], 3)}), flush=True)


def varlen_legs(ctx, k, reps, warmup):
    import ctypes as C
    import hashlib

    from sha2_on_cq_halo2_amd import sha256_circuit as SC
    from sha2_on_cq_halo2_amd.api import Sha256BatchCircuit, Sha256VarCircuit

    blocks_list, rows, usable = [], 0, SC.usable_rows(k)
    while rows + SC.rows_for((1, 2, 4, 8)[len(blocks_list) % 4]) <= usable:  # segments of 1, 2, 4, 8 blocks in turn
        blocks_list.append((1, 2, 4, 8)[len(blocks_list) % 4])
        rows += SC.rows_for(blocks_list[-1])
    # mixed lengths: every fourth message fills its segment, the others end anywhere in it (the empty message included)
    lengths = [64 * b - 9 if j % 4 == 3 else (0x9E3779B1 * j) % (64 * b - 8) for j, b in enumerate(blocks_list)]
    mixed = [bytes((i + j) % 251 for i in range(n_)) for j, n_ in enumerate(lengths)]
    full = [bytes((i + j) % 251 for i in range(64 * b - 9)) for j, b in enumerate(blocks_list)]  # what a fixed-length batch takes
    for name, make, arg in (("Sha256VarCircuit", lambda: Sha256VarCircuit(ctx, k, blocks_list), mixed),
                            ("Sha256BatchCircuit, same block counts", lambda: Sha256BatchCircuit(ctx, k, blocks_list), full)):
        t0 = time.perf_counter()
        c = make()
        row = {"circuit": name, "k": k, "segments": len(blocks_list), "blocks": sum(blocks_list), "rows": c.rows,
               "message_bytes": sum(len(m) for m in arg), "fixed_columns": c.cs.num_fixed_columns, "gates": len(c.cs.gates),
               "proof_bytes": c.pk.proof_size, "keygen_s": round(time.perf_counter() - t0, 2)}
        assert c.check(arg) == (0, []) and c.digests == [hashlib.sha256(m).digest() for m in arg]
        ptrs, seed = [b.ptr for b in c.cols], [0]
        arr = (C.c_void_p * len(ptrs))(*ptrs)

        def call():  # the entry point alone: the bytes (or words) of the last synthesize are still on the device
            c._call(arr)
            ctx.sync()

        def prove():
            seed[0] += 1
            c.pk.create_proof_dev(ptrs, seed=seed[0], instances=c.instances)

        timed(row, (("synthesize_ms", lambda: c.synthesize(arg)), ("synthesize_call_ms", call),
                    ("check_ms", lambda: c.pk.check_witness(ptrs, instances=c.instances, max_failures=0)), ("proof_ms", prove)), reps, warmup)
        c.close()
        print(json.dumps(row), flush=True)


def states_legs(ctx, k, reps, warmup):
    import ctypes as C

    import numpy as np

    from sha2_on_cq_halo2_amd import sha256_circuit as SC
    from sha2_on_cq_halo2_amd import sha256_segments as SS

    n, count = 1 << k, SC.usable_rows(k) // SC.rows_for(1)
    cols = [ctx.alloc(32 * n) for _ in range(SC.ADVICE_COLUMNS)]
    arr = (C.c_void_p * len(cols))(*[b.ptr for b in cols])
    words = np.arange(24 * count, dtype=np.uint32) * np.uint32(0x9E3779B1)  # per segment 8 state words, then 16 message words
    words_dev, digests_dev = ctx.to_device(words), ctx.alloc(32 * count)
    blocks = np.ones(count, dtype=np.uint32)
    sources = (24 * np.arange(count, dtype=np.uint32)[:, None] + 8 + np.arange(16, dtype=np.uint32)).reshape(-1).copy()
    iv = np.full(8 * count, SS.SOURCE_IV, dtype=np.uint32)
    wired = (24 * np.arange(count, dtype=np.uint32)[:, None] + np.arange(8, dtype=np.uint32)).reshape(-1).copy()

    def old():
        ctx._chk(ctx.lib.cq_sha256_synthesize_segments_dev(ctx.h, 12, blocks.ctypes.data, count, sources.ctypes.data, words_dev.ptr, len(words), n, arr,
                                                           digests_dev.ptr))
        ctx.sync()

    def states(init):
        def call():
            ctx._chk(ctx.lib.cq_sha256_synthesize_states_dev(ctx.h, 12, blocks.ctypes.data, count, sources.ctypes.data, None, 0,
                                                             None if init is None else init.ctypes.data, words_dev.ptr, len(words), n, arr,
                                                             digests_dev.ptr))
            ctx.sync()
        return call

    row = {"states": "entry point + sync, one-block segments, no key", "k": k, "segments": count}
    timed(row, (("segments_dev_ms", old), ("states_dev_null_ms", states(None)), ("states_dev_all_iv_ms", states(iv)),
                ("states_dev_private_states_ms", states(wired)), ("segments_dev_again_ms", old)), reps, warmup)
    print(json.dumps(row), flush=True)
    for b in cols + [words_dev, digests_dev]:
        b.close()


def hmac_legs(ctx, k, reps, warmup):
    import ctypes as C
    import hashlib
    import hmac

    import numpy as np

    from sha2_on_cq_halo2_amd import sha256_circuit as SC
    from sha2_on_cq_halo2_amd import sha256_segments as SS
    from sha2_on_cq_halo2_amd.api import Sha256SegmentsCircuit

    key_bytes, message_bytes = 32, 52  # one message block behind the key block
    one = SS.hmac_sha256(key_bytes, message_bytes)
    count, nvars = SC.usable_rows(k) // SS.rows_for(one), key_bytes // 4

    def moved(s, i, strip):  # HMAC i of the plan: its own vars and segments; `strip`: the Xor words as Private words
        if isinstance(s, SS.Xor):
            return SS.PRIVATE if strip else SS.Xor(moved(s.x, i, strip), moved(s.y, i, strip))
        if isinstance(s, SS.Var):
            return SS.Var(s.index + nvars * i)
        return SS.DigestWord(s.segment + 2 * i, s.word) if isinstance(s, SS.DigestWord) else s

    def repeated(strip):
        segs = tuple(SS.Segment(seg.blocks, tuple(moved(s, i, strip) for s in seg.sources)) for i in range(count) for seg in one.segments)
        return SS.Plan(segs, tuple(2 * i + 1 for i in range(count)))

    keys = [hashlib.sha256(b"key %d" % i).digest() for i in range(count)]
    messages = [bytes((i + 3 * j) % 256 for j in range(message_bytes)) for i in range(count)]
    words = lambda data: list(np.frombuffer(data, dtype=">u4"))
    n = 1 << k
    cols = [ctx.alloc(32 * n) for _ in range(SC.ADVICE_COLUMNS)]
    arr = (C.c_void_p * len(cols))(*[b.ptr for b in cols])
    row = {"hmac": "independent HMAC-SHA-256, 32-byte key, 52-byte message", "k": k, "hmacs": count, "segments": 2 * count, "blocks": 4 * count,
           "xor_units": 2 * nvars * count, "rows": count * SS.rows_for(one)}
    legs = []
    for strip in (False, True):
        plan = repeated(strip)
        low = SS.lower(plan)
        if strip:  # the key block's words are private words, in word order before the message's
            values = [x for i in range(count) for x in ([w ^ SS.HMAC_IPAD for w in words(keys[i])] + words(messages[i]), [w ^ SS.HMAC_OPAD for w in words(keys[i])])]
            buf = SS.word_buffer(low, values)
        else:
            buf = SS.word_buffer(low, [x for i in range(count) for x in (words(messages[i]), [])], [w for key in keys for w in words(key)])
        words_dev, digests_dev = ctx.to_device(buf), ctx.alloc(32 * len(low.seg_blocks) + 4 * len(low.xors))

        def call(low=low, words_dev=words_dev, digests_dev=digests_dev, strip=strip):
            if strip:
                ctx._chk(ctx.lib.cq_sha256_synthesize_states_dev(ctx.h, 12, low.seg_blocks.ctypes.data, len(low.seg_blocks), low.sources.ctypes.data,
                                                                 None, 0, None, words_dev.ptr, low.words_len, n, arr, digests_dev.ptr))
            else:
                ctx._chk(ctx.lib.cq_sha256_synthesize_xors_dev(ctx.h, 12, low.seg_blocks.ctypes.data, len(low.seg_blocks), low.sources.ctypes.data,
                                                               None, 0, None, low.xors.ctypes.data, len(low.xors), words_dev.ptr, low.words_len, n,
                                                               arr, digests_dev.ptr))
            ctx.sync()

        call()
        tags = digests_dev.download((2 * count, 8), np.uint32)[1::2].astype(">u4")
        assert [t.tobytes() for t in tags] == [hmac.new(key, m, "sha256").digest() for key, m in zip(keys, messages)]
        legs.append(("states_dev_private_key_blocks_ms" if strip else "xors_dev_ms", call))
    timed(row, legs + [("xors_dev_again_ms", legs[0][1])], reps, warmup)
    for b in cols:
        b.close()
    t0 = time.perf_counter()
    c = Sha256SegmentsCircuit(ctx, k, repeated(False))
    row["keygen_s"] = round(time.perf_counter() - t0, 2)
    values, shared = [x for i in range(count) for x in (words(messages[i]), [])], [w for key in keys for w in words(key)]
    assert c.check(values, shared) == (0, [])
    ptrs, seed = [b.ptr for b in c.cols], [0]

    def prove():
        seed[0] += 1
        c.pk.create_proof_dev(ptrs, seed=seed[0], instances=c.instances)

    def synthesize():
        c.synthesize(values, shared)
        ctx.sync()

    timed(row, (("synthesize_ms", synthesize), ("check_ms", lambda: c.pk.check_witness(ptrs, instances=c.instances, max_failures=0)),
                ("proof_ms", prove)), reps, warmup)
    row["proof_bytes"] = c.pk.proof_size
    c.close()
    print(json.dumps(row), flush=True)


def stream_legs(ctx, k, reps, warmup):
    import hashlib

    from sha2_on_cq_halo2_amd import sha256_circuit as SC
    from sha2_on_cq_halo2_amd.api import Sha256Circuit, Sha256Stream, link

    blocks = SC.max_blocks(k)
    t0 = time.perf_counter()
    s = Sha256Stream(ctx, k, blocks, k, blocks)
    keygen_s = time.perf_counter() - t0
    msg = bytes((i * 7 + i // 251) % 256 for i in range(1 << 20))
    out = s.prove(msg)
    assert link([inst for _, inst in out], blocks, blocks) == (hashlib.sha256(msg).digest(), len(msg))
    row = {"circuit": "Sha256Stream", "k": k, "body_blocks": blocks, "tail_max_blocks": blocks, "message_bytes": len(msg), "proofs": len(out),
           "proof_bytes": [s.body.pk.proof_size, s.tail.pk.proof_size], "keygen_s": round(keygen_s, 2)}
    row["prove_total_ms"], row["prove_total_ms_range"] = median_ms(lambda: s.prove(msg), 3, 1)
    row["per_proof_ms"] = round(row["prove_total_ms"] / len(out), 3)
    s.close()
    c = Sha256Circuit(ctx, k)
    one = bytes(i % 251 for i in range(64 * c.blocks - 9))
    row["sha256circuit_prove_ms"], row["sha256circuit_prove_ms_range"] = median_ms(lambda: c.prove(one), reps, warmup)
    c.close()
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="14,18")
    ap.add_argument("--segments-k", type=int, default=0)
    ap.add_argument("--path-k", type=int, default=0)
    ap.add_argument("--varlen-k", type=int, default=0)
    ap.add_argument("--states-k", type=int, default=0)
    ap.add_argument("--stream-k", type=int, default=0)
    ap.add_argument("--hmac-k", type=int, default=0)
    ap.add_argument("--sweep", default="1,2,4,8,16,32,64,128,256,512")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert args.reps >= 10, "a median of at least 10 runs"
    import hashlib

    from sha2_on_cq_halo2_amd import Context
    from sha2_on_cq_halo2_amd.api import Sha256Circuit
    from sha2_on_cq_halo2_amd.sha_circuit import ShaPlonkWorkload

    ctx = Context(0)
    for k in (int(s) for s in args.sizes.split(",") if s):
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
    if args.segments_k:
        segment_legs(ctx, args.segments_k, args.sweep, args.reps, args.warmup)
    if args.path_k:
        path_legs(ctx, args.path_k, args.reps, args.warmup)
    if args.varlen_k:
        varlen_legs(ctx, args.varlen_k, args.reps, args.warmup)
    if args.states_k:
        states_legs(ctx, args.states_k, args.reps, args.warmup)
    if args.stream_k:
        stream_legs(ctx, args.stream_k, args.reps, args.warmup)
    if args.hmac_k:
        hmac_legs(ctx, args.hmac_k, args.reps, args.warmup)
    ctx.close()


if __name__ == "__main__":
    main()

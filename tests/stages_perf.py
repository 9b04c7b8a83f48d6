"""Measurement, not a test: the proof of ShaPlonkWorkload composed from the stand-alone stage calls (tests/stages_helpers.py,
ComposedProver) against cq_create_proof of the same key and RNG stream.  usage, from the repository root:
python tests/stages_perf.py [k]   (profiles/r14_stage_abi.txt keeps the k = 18 figures)"""
import sys, time
import numpy as np
sys.path.insert(0, ".")
from oracle import bn254 as B
from sha2_on_cq_halo2_amd import Context
from sha2_on_cq_halo2_amd.api import fr_to_mont
from sha2_on_cq_halo2_amd.sha_circuit import ShaPlonkWorkload
from tests.stages_helpers import ComposedProver

k = int(sys.argv[1]) if len(sys.argv) > 1 else 18
n = 1 << k
ctx = Context(0)
wl = ShaPlonkWorkload(ctx, k, seed=0x5348413243515F)
pk = wl.pk
rows = pk.usable_rows - 1
qcol = np.zeros((n, 4), dtype=np.uint64); qcol[:rows] = fr_to_mont(1)
mapping = np.zeros((2, n, 2), dtype=np.uint32)
mapping[0, :, 0], mapping[1, :, 0] = 0, 1
mapping[:, :, 1] = np.arange(n, dtype=np.uint32)
r = np.arange(rows, dtype=np.uint32)
mapping[1, r, 0], mapping[1, r, 1] = 0, r + 1
mapping[0, r + 1, 0], mapping[0, r + 1, 1] = 1, r
words = B.Xoshiro256ss(5).words(8 * (n + 400))
host = [c.download((n, 4)) for c in wl.cols]
for opener in ("gwc", "shplonk"):
    pk.set_opener(opener)
    whole = pk.create_proof_dev([c.ptr for c in wl.cols], rng_words=words)
    ts = []
    for _ in range(5):
        ctx.sync(); t0 = time.perf_counter()
        pk.create_proof_dev([c.ptr for c in wl.cols], rng_words=words)
        ctx.sync(); ts.append((time.perf_counter() - t0) * 1e3)
    cp = ComposedProver(ctx, pk, [qcol], mapping)
    res = []
    for _ in range(2):
        cols = [ctx.to_device(h) for h in host]
        cp.seconds_in_library = 0.0
        ctx.sync(); t0 = time.perf_counter()
        proof = cp.prove(cols, words, 0xC0FFEE + k, opener)
        ctx.sync(); res.append(((time.perf_counter() - t0) * 1e3, cp.seconds_in_library * 1e3))
    print(f"k={k} {opener}: composed == whole: {proof == whole}; cq_create_proof ms {sorted(ts)}; "
          f"composed (total ms, ms inside library calls) {res}", flush=True)

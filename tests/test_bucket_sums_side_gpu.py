"""GPU: the bucket-sum launch of a proof beside the launch that commits [m] ("the side stream").

The sums are the same group elements whatever stream forms them, so every check is on proof BYTES: side placement
against `CQ_BUCKET_SUMS_SIDE=0` (the launch in front, on the main stream; the switch is an environment variable, so that
half runs in ONE fresh child process for all cases) and against the oracle the existing proof tests compare with; proofs
back to back on one context against fresh contexts (a stale workspace, a stale index region, a missed join); the paths
around it: the late-m fork beside round 1's launch, a key with gates and a permutation under both openers, a lookup
error between the fork and the join, lanes, and the profiling brackets.

Circuits: the SHA workloads at k = 12 (the 2^12-entry tables, n = 4096: the smallest size they are built at with these
tables in the suite) and the tiny oracle fixtures.  A key takes at most CQ_MAX_LOOKUPS = 16 lookups and a bucket-sum launch
MSM_MAX_BATCH / 2 = 16 of them, so a proof cannot be made to issue two such launches: the widest case here is the full
single launch of 16 lookups (32 arrays)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import bn254 as B
from oracle import cbind as OC
from oracle import cq_prover as CP
from tests.plonk_fixtures import oracle_env

from .test_plonk_gpu import _backend_pk
from .test_prover_gpu import _prove_both, _setup

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 12
PROF_MSM_ACCUMULATE, PROF_MSM_ENTRIES = 1, 3


def _spread(x):
    r = 0
    for i in range(16):
        r |= ((x >> i) & 1) << (2 * i)
    return r


_wide_cache = {}


def _wide_env(ctx):
    """16 width-2 lookups at k = 5: the widest bucket-sum launch a key can ask for (built once per context, never modified)."""
    if id(ctx) not in _wide_cache:
        _wide_cache[id(ctx)] = _build_wide_env(ctx)
    return _wide_cache[id(ctx)]


def _build_wide_env(ctx):
    k, nbits, pairs = 5, 5, 16
    N, n = 1 << nbits, 1 << k
    tv = {"dense": list(range(N)), "spread": [_spread(i) for i in range(N)]}
    env = _setup(ctx, k, tv, [[(2 * p, "dense"), (2 * p + 1, "spread")] for p in range(pairs)], 2 * pairs, 100 + k, srs_len=max(N, n))
    rng = B.Xoshiro256ss(k)
    advice = []
    for p in range(pairs):
        vals = [rng.next_u64() % N for _ in range(n - 6 - 3)]
        advice += [vals, [_spread(v) for v in vals]]
    return env, advice


def _late_m_fixture():
    """three phases and a static lookup: `early_m` is false, the fork sits beside round 1's launch"""
    return oracle_env(5, phases=True, with_lookup=True)


def _late_m_proof(ctx, fx):
    n = 1 << 5
    cs = fx["circuit"]
    gpk, _ = _backend_pk(ctx, fx, 5, fx["s"], b0=fx["pk"].b0_g1_bound)
    bufs = [ctx.to_device(B.to_mont_limbs([0] * n if callable(col) else list(col) + [0] * (n - len(col)))) for col in fx["advice"]]

    def phase_fn(phase, challenges):
        out = {}
        for c_, col in enumerate(fx["advice"]):
            if callable(col) and cs.phase_of(c_) == phase:
                vals = col(challenges)
                out[c_] = B.to_mont_limbs(list(vals) + [0] * (n - len(vals)))
        return out

    return gpk.create_proof_phases(bufs, phase_fn, seed=41, instances=[B.to_mont_limbs(i) for i in fx["instances"]])


def _profile_counts(ctx, wl):
    """(accumulate launches, entries) of one proof"""
    ctx.profile_enable(True)
    try:
        ctx.profile_read(PROF_MSM_ACCUMULATE)
        ctx.profile_read(PROF_MSM_ENTRIES)
        wl.prove(seed=9)
        return [ctx.profile_read(PROF_MSM_ACCUMULATE)[1], ctx.profile_read(PROF_MSM_ENTRIES)[1]]
    finally:
        ctx.profile_enable(False)


def _cases(ctx):
    """Every proof both halves compare, by name (hex), with whatever placement the environment selects."""
    from sha2_on_cq_halo2_amd.sha_circuit import ShaCqWorkload, ShaPlonkWorkload

    out = {}
    wl = ShaCqWorkload(ctx, K, pairs=2)
    out["sha"] = wl.prove(seed=9).hex()
    out["profile"] = _profile_counts(ctx, wl)
    wl.close()
    wl = ShaPlonkWorkload(ctx, K, pairs=2)
    for opener in ("gwc", "shplonk"):
        wl.pk.set_opener(opener)
        out["plonk-" + opener] = wl.prove(seed=4).hex()
    wl.close()
    env, advice = _wide_env(ctx)
    n = 1 << 5
    words = B.Xoshiro256ss(1005).words(8 * (len(advice) * 8 + n + 16))
    out["wide"] = env["gpk"].create_proof([B.to_mont_limbs(list(c) + [0] * (n - len(c))) for c in advice], rng_words=words).hex()
    out["late-m"] = _late_m_proof(ctx, _late_m_fixture()).hex()
    return out


def _child_main():
    from sha2_on_cq_halo2_amd import Context

    ctx = Context(0)
    print("CASES " + json.dumps(_cases(ctx)), flush=True)
    ctx.close()


@functools.lru_cache(maxsize=1)
def _main_stream_cases():
    """the cases with the launch on the main stream, from one fresh process (never modified)"""
    env = dict(os.environ, CQ_BUCKET_SUMS_SIDE="0")
    r = subprocess.run([sys.executable, "-c", "from tests.test_bucket_sums_side_gpu import _child_main; _child_main()"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("CASES ")][-1]
    return json.loads(line[len("CASES "):])


@pytest.fixture(scope="module")
def side_cases(ctx):
    assert os.environ.get("CQ_BUCKET_SUMS_SIDE", "1") != "0", "this half wants the side placement"
    return _cases(ctx)


@pytest.mark.parametrize("case", ["sha", "plonk-gwc", "plonk-shplonk", "wide", "late-m"])
def test_side_and_main_stream_proofs_are_identical(side_cases, case):
    assert side_cases[case] == _main_stream_cases()[case]


def test_profile_counts_do_not_depend_on_the_placement(side_cases):
    """PROF_MSM_ACCUMULATE launches and PROF_MSM_ENTRIES per proof: the side launch is counted, once"""
    calls, entries = side_cases["profile"]
    assert calls > 0 and entries > 0
    assert [calls, entries] == _main_stream_cases()["profile"]


def test_sha_proof_equals_the_c_restatement(ctx, side_cases):
    from sha2_on_cq_halo2_amd.api import fr_to_mont
    from sha2_on_cq_halo2_amd.sha_circuit import ShaCqWorkload, small_to_mont, spread16

    wl = ShaCqWorkload(ctx, K, pairs=2)
    n, N = 1 << K, wl.cfg.size
    g, gl = wl.params.download()
    tl, t0 = wl.cfg.download()
    idx = np.arange(N)
    cproof = OC.create_proof(K, 4, [[(0, 0), (1, 1)], [(2, 0), (3, 1)]], [small_to_mont(idx), small_to_mont(spread16(idx))],
                             [wl.dense.download_qs(), wl.spread.download_qs()], g, gl, tl, t0, g[1:], OC.keygen_l_active(K, 5),
                             fr_to_mont(0xC0FFEE + K), [c.download((n, 4)) for c in wl.cols], 9)
    wl.close()
    assert bytes.fromhex(side_cases["sha"]) == cproof


def test_widest_launch_equals_the_oracle(ctx, side_cases):
    env, advice = _wide_env(ctx)
    tr, proof = _prove_both(env, advice, 1005)
    assert proof == tr.proof and proof.hex() == side_cases["wide"]


def test_late_m_proof_equals_the_oracle(ctx, side_cases):
    fx = _late_m_fixture()
    tr = CP.create_proof(fx["params"], fx["pk"], fx["advice"], B.Xoshiro256ss(41), instances=fx["instances"])
    assert bytes.fromhex(side_cases["late-m"]) == tr.proof


def _rotated(ctx, wl, i):
    """witness i: the base witness with its usable rows rotated (still in the tables)"""
    n, u = 1 << wl.k, wl.pk.usable_rows
    cols = []
    for c in wl.cols:
        a = c.download((n, 4))
        a[:u] = np.roll(a[:u], 11 * i, axis=0)
        cols.append(ctx.to_device(a))
    return cols


def test_back_to_back_proofs_equal_those_of_fresh_contexts(ctx):
    from sha2_on_cq_halo2_amd import Context
    from sha2_on_cq_halo2_amd.sha_circuit import ShaCqWorkload

    wl = ShaCqWorkload(ctx, K, pairs=2)
    witnesses = [_rotated(ctx, wl, i) for i in range(3)]
    got = [wl.pk.create_proof_dev([c.ptr for c in w], seed=50 + i) for i, w in enumerate(witnesses)]  # no host wait in between but the proofs' own
    wl.close()
    assert len(set(got)) == 3
    for i in range(3):
        fresh = Context(0)
        fwl = ShaCqWorkload(fresh, K, pairs=2)
        want = fwl.pk.create_proof_dev([c.ptr for c in _rotated(fresh, fwl, i)], seed=50 + i)
        fwl.close()
        fresh.close()
        assert got[i] == want, "proof %d" % i


def test_lookup_error_then_a_good_witness_on_the_same_context(ctx):
    """The error is read after the advice launch, with the side launch queued: the call joins it, and the next proof is right."""
    from sha2_on_cq_halo2_amd import CqError
    from sha2_on_cq_halo2_amd.sha_circuit import ShaCqWorkload

    wl = ShaCqWorkload(ctx, K, pairs=2)
    n = 1 << K
    ref = wl.prove(seed=9)
    good = wl.cols[0].download((n, 4))
    bad = good.copy()
    bad[3] = B.to_mont_limbs([4097])[0]  # one value outside the table
    wl.cols[0].upload(bad)
    with pytest.raises(CqError) as e:
        wl.prove(seed=9)
    assert e.value.code == -4
    wl.cols[0].upload(good)
    assert wl.prove(seed=9) == ref
    wl.close()


def test_two_lanes_first_proof_equals_the_single_proof(ctx):
    from sha2_on_cq_halo2_amd.sha_circuit import ShaCqWorkload

    wl = ShaCqWorkload(ctx, K, pairs=2)
    witnesses = [_rotated(ctx, wl, i) for i in range(3)]
    singles = [wl.pk.create_proof_dev([c.ptr for c in w], seed=70 + i) for i, w in enumerate(witnesses)]
    got = wl.pk.create_proof_batch([[c.ptr for c in w] for w in witnesses], [70 + i for i in range(3)], lanes=2)
    wl.close()
    assert got[0] == singles[0]
    assert got == singles

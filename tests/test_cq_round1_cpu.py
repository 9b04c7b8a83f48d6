"""CPU: tests/tablehash_model.py against the compiled `hash_fr` of csrc/tablehash.hpp, and the properties of the colliding
tables that tests/test_cq_round1_gpu.py relies on.  If the hash changed, the first test fails; if the searches stopped
producing collisions, the others do -- the GPU tests could otherwise go on passing on tables that no longer collide."""
import os
import subprocess
import time

import pytest

from oracle import bn254 as B
from tests import tablehash_model as M

P = B.R_MOD
SIZES = (64, 512)


def test_model_hash_equals_the_compiled_hash(tmp_path):
    """g++ on tests/host/tablehash_check.cpp (HIP-free): small integers, p - 1, random elements and every value the
    searches return."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "tablehash_check")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "sha2_on_cq_halo2_amd", "csrc"),
                        os.path.join(root, "tests", "host", "tablehash_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rng = B.Xoshiro256ss(77)
    values = list(range(40)) + [P - 1, P - 2, (P - 1) // 2, 1 << 253] + [B.fr_random(rng) for _ in range(200)]
    for N in SIZES:
        t = M.tables_for(N)
        values += t["wrap"][:40] + t["wrap2"][:20] + t["adjacent"][:40] + t["random"][:10] + list(M.absent_values(N).values())
    words = M.mont_words(values)
    text = "".join(" ".join("%08x" % w for w in row) + "\n" for row in words)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = [int(line, 16) for line in r.stdout.split()]
    assert len(values) > 400 and got == [int(h) for h in M.hash_fr(words)]
    assert len(set(got)) > 300  # not a constant: the vectors tell hashes apart
    # an incomplete element is an error, not a shorter answer
    r = subprocess.run([exe], input="1 2 3\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 1


def test_nslots_and_home():
    assert [M.nslots_for(N) for N in (1, 2, 16, 64, 65, 512)] == [4, 8, 64, 256, 512, 2048]
    for v in (0, 1, P - 1, 12345678901234567890):
        words = M.mont_words([v])
        assert M.home(v, 256) == int(M.hash_fr(words)[0]) % 256 == int(M.hash_fr(words[0])[0]) % 256
        assert M.from_words(words[0]) == v


@pytest.mark.parametrize("N", SIZES)
def test_tables_collide_as_prescribed(N):
    nslots = M.nslots_for(N)
    t = M.tables_for(N)
    for name, vals in t.items():
        assert len(vals) == N and len(set(vals)) == N and all(0 <= v < P for v in vals), name
    homes = {name: [M.home(v, nslots) for v in vals] for name, vals in t.items()}
    assert homes["wrap"] == [nslots - 3] * N and homes["wrap2"] == [nslots - 3] * N
    assert not set(t["wrap"]) & set(t["wrap2"])
    # the cluster of N slots from nslots - 3 on wraps past the end of the slot array
    assert N > 3 and (nslots - 3) + N > nslots
    assert homes["adjacent"] == [7 + i // 2 for i in range(N)]
    assert 7 + N <= nslots - 3  # ... and that cluster, slots 7 .. 7 + N - 1, does not wrap
    assert len(set(homes["random"])) > N // 2  # the control is spread out


@pytest.mark.parametrize("N", SIZES)
def test_absent_values_are_absent_and_start_where_prescribed(N):
    nslots = M.nslots_for(N)
    t = M.tables_for(N)
    a = M.absent_values(N)
    taken = set(t["wrap"]) | set(t["wrap2"])
    assert len(set(a.values())) == 4 and all(0 <= v < P and v not in taken for v in a.values())
    assert [M.home(a[name], nslots) for name in ("head", "empty", "top", "low")] == [nslots - 3, nslots // 2, nslots - 3, nslots - 3]
    # nslots / 2 is outside the cluster nslots - 3 .. nslots - 1, 0 .. N - 4
    assert N - 4 < nslots // 2 < nslots - 3
    entry = M.mont_words([t["wrap"][N // 2]])[0]
    assert (M.mont_words([a["top"]])[0] != entry).nonzero()[0].tolist() == [7]
    assert (M.mont_words([a["low"]])[0] != entry).nonzero()[0].tolist() == [0]


def test_searches_are_deterministic_and_quick():
    t0 = time.perf_counter()
    again = M.one_home(512, 2045), M.adjacent_homes(512, 7), M.absent_with_home(2045, (), 2048)
    dt = time.perf_counter() - t0
    assert again[0] == M.tables_for(512)["wrap"] and again[1] == M.tables_for(512)["adjacent"]
    assert again[2] == M.absent_with_home(2045, (), 2048)
    assert M.absent_with_home(2045, [again[2]], 2048) != again[2]
    assert M.one_home(64, 253, seed=11) == M.tables_for(64)["wrap2"] != M.one_home(64, 253)
    print("one_home(512) + adjacent_homes(512) + absent_with_home: %.3f s" % dt)
    assert dt < 5.0  # about 10^6 hashes; a second each is the budget, this leaves room for a loaded machine

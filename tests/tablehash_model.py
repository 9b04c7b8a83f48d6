"""The static table's value -> slot hash (csrc/tablehash.hpp `hash_fr`, csrc/cq.hip `cq_table_build_index`) restated with
numpy uint32 arithmetic, and seeded searches for field values with prescribed home slots: tables whose entries collide on
purpose, so that probe chains are long, wrap past the end of the slot array and merge.

A value is a canonical Python integer below the modulus; the hash reads its Montgomery form v * 2^256 mod r as eight
32-bit words, least significant first.  tests/test_cq_round1_cpu.py pins `hash_fr` to the compiled function.
"""
import numpy as np

from oracle import bn254 as B

P = B.R_MOD
R_INV = pow(1 << 256, -1, P)
TOP_WORD = P >> 224  # a Montgomery form whose top word is below this one is below the modulus


def mont_words(values) -> np.ndarray:
    """canonical integers -> uint32[len, 8], the words `hash_fr` reads"""
    return np.ascontiguousarray(B.to_mont_limbs([int(v) for v in values])).view(np.uint32).reshape(-1, 8)


def from_words(words) -> int:
    """eight Montgomery words -> the canonical integer"""
    m = sum(int(w) << (32 * i) for i, w in enumerate(words))
    assert m < P
    return m * R_INV % P


def hash_fr(limbs) -> np.ndarray:
    """`hash_fr` over uint32[..., 8] Montgomery words -> uint32[...]"""
    limbs = np.asarray(limbs, dtype=np.uint32)
    h = np.full(limbs.shape[:-1] if limbs.ndim > 1 else (1,), 0x9E3779B9, dtype=np.uint32)
    for i in range(8):
        h ^= limbs[..., i]
        h *= np.uint32(0x85EBCA6B)  # wraps modulo 2^32 on arrays
        h ^= h >> np.uint32(15)
    return h


def nslots_for(N: int) -> int:
    """slots of a table of N values: the smallest power of two >= 4 and >= 4 N (`cq_table_build_index`)"""
    nslots = 4
    while nslots < 4 * N:
        nslots <<= 1
    return nslots


def home(value: int, nslots: int) -> int:
    """the slot a value's probe chain starts at"""
    return int(hash_fr(mont_words([value]))[0]) & (nslots - 1)


# ---- searches ---------------------------------------------------------------------------------------------------------
def _splitmix64(x: np.ndarray) -> np.ndarray:
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _candidates(seed: int, chunk: int, count: int) -> np.ndarray:
    """uint32[count, 8]: Montgomery words of distinct field elements, a pure function of (seed, chunk)"""
    ctr = (np.uint64(seed) << np.uint64(48)) + np.uint64(chunk) * np.uint64(count * 4) + np.arange(count * 4, dtype=np.uint64)
    w = _splitmix64(ctr).view(np.uint32).reshape(count, 8).copy()  # a bijection of the counter: no two rows are equal
    w[:, 7] %= np.uint32(TOP_WORD)
    return w


def _with_homes(homes, per_home: int, nslots: int, seed: int, exclude=()):
    """{home: [per_home canonical values]} for every home asked for, in the order the candidate stream gives them"""
    found = {h: [] for h in homes}
    missing = len(found) * per_home
    exclude = set(exclude)
    chunk = 0
    while missing:
        assert chunk < 256, "search did not finish"
        w = _candidates(seed, chunk, 1 << 16)
        hm = hash_fr(w) & np.uint32(nslots - 1)
        for i in np.nonzero(np.isin(hm, list(found)))[0]:
            got = found[int(hm[i])]
            if len(got) < per_home:
                v = from_words(w[i])
                if v not in exclude:
                    got.append(v)
                    missing -= 1
        chunk += 1
    return found


def one_home(N: int, slot: int, seed: int = 1):
    """N distinct values whose home is `slot` of a table of N entries: one cluster of N slots from `slot` on"""
    return _with_homes([slot], N, nslots_for(N), seed)[slot]


def adjacent_homes(N: int, first: int, seed: int = 2):
    """N distinct values with homes first, first + 1, ... (modulo the slot count), two each: the clusters merge into one"""
    assert N % 2 == 0
    nslots = nslots_for(N)
    homes = [(first + i) % nslots for i in range(N // 2)]
    found = _with_homes(homes, 2, nslots, seed)
    return [v for h in homes for v in found[h]]


def absent_with_home(slot: int, exclude, nslots: int, seed: int = 3) -> int:
    """a value outside `exclude` whose home is `slot`"""
    return _with_homes([slot], 1, nslots, seed, exclude)[slot][0]


def near_miss(value: int, word: int, slot: int, nslots: int) -> int:
    """a value whose Montgomery form equals `value`'s in every 32-bit word but `word`, with home `slot`: a probe from `slot`
    that reaches `value` must compare all 256 bits to tell them apart"""
    w = mont_words([value])[0]
    assert w[7] < TOP_WORD
    cand = np.tile(w, (1 << 16, 1))
    cand[:, word] = np.arange(1 << 16, dtype=np.uint32) * np.uint32(0x9E3779B1)
    if word == 7:
        cand[:, 7] %= np.uint32(TOP_WORD)
    ok = ((hash_fr(cand) & np.uint32(nslots - 1)) == slot) & (cand[:, word] != w[word])
    return from_words(cand[np.nonzero(ok)[0][0]])


# ---- the tables of tests/test_cq_round1_gpu.py ----------------------------------------------------------------------------
_TABLES = {}


def tables_for(N: int) -> dict:
    """name -> N canonical values: "wrap" and "wrap2", two different tables that are one cluster each from slot nslots - 3
    on (it wraps past the end of the slot array); "adjacent", homes 7, 8, ... with two values each; "random", a control"""
    if N not in _TABLES:
        nslots = nslots_for(N)
        rng = B.Xoshiro256ss(0x7AB1E + N)
        _TABLES[N] = dict(wrap=one_home(N, nslots - 3, seed=1), wrap2=one_home(N, nslots - 3, seed=11),
                          adjacent=adjacent_homes(N, 7), random=[B.fr_random(rng) for _ in range(N)])
    return _TABLES[N]


def absent_values(N: int) -> dict:
    """name -> a value that is in neither "wrap" table of N entries: "head", its home is the head of the cluster, so the probe
    walks all N entries and the wrap to the first empty slot; "empty", its home is an empty slot; "top" / "low", equal to
    entry N / 2 of the "wrap" cluster in all but the top / lowest word, home at the head of the cluster"""
    t = tables_for(N)
    nslots = nslots_for(N)
    taken = t["wrap"] + t["wrap2"]
    entry = t["wrap"][N // 2]
    return dict(head=absent_with_home(nslots - 3, taken, nslots), empty=absent_with_home(nslots // 2, taken, nslots),
                top=near_miss(entry, 7, nslots - 3, nslots), low=near_miss(entry, 0, nslots - 3, nslots))

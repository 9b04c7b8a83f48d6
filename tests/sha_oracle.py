"""What the SHA circuit tests share when they hand a circuit to the oracle: the package's constraint system restated in
oracle/plonk.py expressions (for the oracle's verifier and for tests/witness_check_model.py), a model's column of integers
in Montgomery form, and one 32-byte cell written into a device column."""
import numpy as np

from oracle import bn254 as B
from oracle import cq_prover as CP
from oracle import cq_verifier as CV
from oracle import plonk as PL
from sha2_on_cq_halo2_amd import plonk as GP
from sha2_on_cq_halo2_amd._marshal import fr_to_mont
from sha2_on_cq_halo2_amd.sha256_circuit import _mont_column

KINDS = {GP.COL_ADVICE: PL.ADVICE, GP.COL_FIXED: PL.FIXED, GP.COL_INSTANCE: PL.INSTANCE}


def mont_column(vals) -> np.ndarray:
    """integers below the modulus -> uint64[n, 4] Montgomery limbs, one conversion per distinct value"""
    if max(vals) < 1 << 64:
        return _mont_column(np.array(vals, dtype=np.uint64))
    index, uniq = {}, []
    inv = np.empty(len(vals), dtype=np.int64)
    for i, v in enumerate(vals):
        j = index.get(v)
        if j is None:
            j = index[v] = len(uniq)
            uniq.append(v)
        inv[i] = j
    return np.stack([fr_to_mont(u) for u in uniq])[inv]


def spread(x):
    """bit i -> bit 2i"""
    out = i = 0
    while x >> i:
        out |= ((x >> i) & 1) << (2 * i)
        i += 1
    return out


def oracle_expr(e):
    if e.op == "const":
        return PL.const(e.a)
    if e.op == "query":
        return (PL.adv, PL.fix, PL.inst)[e.a.kind](e.a.index, e.b)
    if e.op == "neg":
        return PL.neg(oracle_expr(e.a))
    if e.op == "scale":
        return PL.scale(oracle_expr(e.a), e.b)
    return (PL.add if e.op == "add" else PL.mul)(oracle_expr(e.a), oracle_expr(e.b))


def oracle_circuit(cs, k, table_name):
    """The constraint system as the oracle's `CqCircuit`; `table_name(table)` names a static table of a lookup."""
    exprs = iter(cs._lookup_exprs)
    lookups = [[(oracle_expr(next(exprs)), table_name(t)) for _, t in lk] for lk in cs.static_lookups]
    queries = {PL.ADVICE: list(cs.advice_queries), PL.FIXED: list(cs.fixed_queries), PL.INSTANCE: list(cs.instance_queries)}
    circ = CP.CqCircuit(k, cs.num_advice_columns, lookups, cs.num_fixed_columns, 1, [oracle_expr(g) for g in cs.gates],
                        [(KINDS[col.kind], col.index) for col in cs.permutation_columns], queries)
    assert circ.degree() == cs.degree() and circ.blinding_factors() == cs.blinding_factors()
    return circ


def verifier(c, seed):
    """The circuit's constraint system restated for the oracle's verifier -> verify(proof, instance words)."""
    names = {id(c.dense): "dense", id(c.spread): "spread"}
    circ = oracle_circuit(c.cs, c.k, lambda t: names[id(t)])
    s = (seed * 0x9E3779B97F4A7C15 + 12345) % B.R_MOD
    N = 1 << c.table_bits
    tv = {"dense": list(range(N)), "spread": [spread(i) for i in range(N)]}
    fcm, pcm = c.pk.vk_commitments()

    def verify(proof, instance_words):
        return CV.verify_proof(proof, circ, c.vk_repr, s, tv, N, 1 << c.k, instances=[list(instance_words)],
                               fixed_commitments=B.points_from_mont_limbs(fcm), perm_commitments=B.points_from_mont_limbs(pcm))

    return verify


def write_cell(c, column, row, value):
    from sha2_on_cq_halo2_amd.api import fr_to_mont

    v = np.ascontiguousarray(fr_to_mont(value), dtype=np.uint64)
    c.ctx._chk(c.ctx.lib.cq_dev_upload(c.ctx.h, c.cols[column].ptr + 32 * row, v.ctypes.data, 32))

"""Proving-key construction (csrc/pk.hip) at k = 5 over a 16-row table: a key that was computed and a key that was read from
a stream are the same key, for every shape of key and both portable formats; every rejection of a description or a stream
keeps its code and text and leaves the context usable; re-tabling for two ranks and back changes no proof.

The yardstick is the oracle: oracle/serde.py serializes the oracle's key (RawBytes), tests/serde_processed_model.py
transcodes that stream to Processed."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

from oracle import bn254 as B
from oracle import cq_prover as CP
from oracle import kzg
from oracle import serde as SD
from tests import serde_processed_model as SM
from tests.plonk_fixtures import TABLE, oracle_env, to_backend_cs

pytestmark = pytest.mark.gpu
K = 5
N_ROWS = 1 << K
VK = 424242
PROCESSED, RAW, RAW_UNCHECKED = 0, 1, 2
SELECTORS = [[(r * 7 + 1) % 3 == 0 for r in range(N_ROWS)], [r % 2 == 1 for r in range(N_ROWS)]]
SEL = SD.pack_selectors(SELECTORS, N_ROWS)
SHAPES = {"cq-only": None, "deg3": dict(), "deg5": dict(degree5=True), "lookup": dict(with_lookup=True),
          "lookup-expr": dict(lookup_expr=True), "plookup": dict(plookup=True)}


def _cq_only_env():
    """A circuit of advice columns and one vector lookup alone (no `cs`): the SRS layout of oracle_env."""
    s = B.fr_random(B.Xoshiro256ss(0x6371))
    table2 = [(3 * v + 1) % B.R_MOD for v in TABLE]
    circuit = CP.CqCircuit(K, 2, [[(0, "t"), (1, "t2")]])
    tsrs = kzg.TableSRS(len(TABLE) - 1, s)
    tables = {"t": TABLE, "t2": table2}
    tabs = {name: kzg.StaticTableValues(v, tsrs.g1) for name, v in tables.items()}
    b0 = kzg._powers_g1(s, 2 * N_ROWS)[N_ROWS + 1:]
    pk = CP.keygen_pk(circuit, tabs, tsrs, b0, VK)
    u = N_ROWS - (circuit.blinding_factors() + 1)
    rows = [(r * 7 + 3) % len(TABLE) for r in range(u)]
    return dict(circuit=circuit, fixed=[], advice=[[TABLE[i] for i in rows], [table2[i] for i in rows]], instances=None, mapping=None,
                tables=tables, s=s, params=kzg.ParamsKZG(K, s), pk=pk)


@functools.lru_cache(maxsize=None)
def _env(shape):
    """Oracle key, its RawBytes stream and the witness of one shape; shared by the cases of that shape, never modified."""
    fx = _cq_only_env() if SHAPES[shape] is None else oracle_env(K, **SHAPES[shape])
    fixed_cm = B.batch_to_affine([fx["params"].commit_lagrange(c) for c in fx["pk"].fixed_values]) if fx["pk"].fixed_values else []
    perm_cm = B.batch_to_affine([fx["params"].commit_lagrange(c) for c in fx["pk"].permutations]) if fx["pk"].permutations else []
    fx["nperm"] = len(perm_cm)
    fx["raw"] = SD.proving_key_to_bytes(fx["pk"], fixed_cm, perm_cm, SELECTORS)
    return fx


class _Backend:
    """The device objects of one shape and the arguments every ProvingKey of that shape takes."""

    def __init__(self, ctx, fx, params=None):
        from sha2_on_cq_halo2_amd import ParamsKZG, StaticTable, TableConfig

        self.ctx, self.fx = ctx, fx
        sm = B.to_mont_limbs([fx["s"]])[0]
        self.sm = sm
        self.params = params or ParamsKZG.setup_from_toxic_waste(ctx, K, sm)
        self.cfg, self.tables, self.b0 = None, {}, None
        if fx["tables"]:
            self.cfg = TableConfig.setup_from_toxic_waste(ctx, len(TABLE), sm)
            self.tables = {name: StaticTable.setup_from_toxic_waste(ctx, B.to_mont_limbs(v), sm) for name, v in fx["tables"].items()}
            self.b0 = B.points_to_mont_limbs(fx["pk"].b0_g1_bound)
        self.general = bool(fx["circuit"].perm_columns)
        self.cs = to_backend_cs(fx["circuit"], self.tables) if self.general else None
        self.lookups = [] if self.general else [[(c, self.tables[t]) for c, t in lk] for lk in fx["circuit"].lookups]
        self.num_advice = 0 if self.general else fx["circuit"].num_advice
        self.vk = B.to_mont_limbs([VK])[0]
        self.cols = [B.to_mont_limbs(list(c) + [0] * (N_ROWS - len(c))) for c in fx["advice"]]
        self.inst = [B.to_mont_limbs(i) for i in fx["instances"]] if fx["instances"] else None

    def create(self, **over):
        from sha2_on_cq_halo2_amd import ProvingKey

        a = dict(params=self.params, k=K, cfg=self.cfg, b0=self.b0, lookups=self.lookups, fixed=[B.to_mont_limbs(c) for c in self.fx["fixed"]],
                 permutation=np.array(self.fx["mapping"], dtype=np.uint32) if self.general else None)
        a.update(over)
        return ProvingKey(self.ctx, a["params"], a["k"], self.num_advice, a["lookups"], a["cfg"], a["b0"], self.vk, cs=self.cs,
                          fixed=a["fixed"] if self.general else None, permutation=a["permutation"])

    def read(self, data, fmt, num_selectors=len(SELECTORS)):
        from sha2_on_cq_halo2_amd import ProvingKey

        return ProvingKey.read(self.ctx, self.params, K, self.num_advice, self.lookups, self.cfg, self.b0, self.vk, data, fmt, cs=self.cs,
                               num_selectors=num_selectors)

    def prove(self, key, seed=3):
        return key.create_proof(self.cols, seed=seed, instances=self.inst)

    def close(self):
        for t in self.tables.values():
            t.close()
        if self.cfg:
            self.cfg.close()
        self.params.close()


@pytest.mark.parametrize("fmt", [RAW, PROCESSED], ids=["raw", "processed"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_created_key_equals_read_key(ctx, shape, fmt):
    """write(created key) is the oracle's serialization of the oracle's key; the key read from those bytes writes them again
    and proves to the same bytes.  (cq-only: l0 / l_last are not kept -- recomputed on write, skipped on read.)"""
    fx = _env(shape)
    want = fx["raw"] if fmt == RAW else SM.pk_raw_to_processed(fx["raw"], fx["nperm"], len(SELECTORS))
    be = _Backend(ctx, fx)
    gpk = be.create()
    assert gpk.serialized_size(fmt, len(SELECTORS)) == len(want)
    assert gpk.write(fmt, SEL, len(SELECTORS)) == want
    rpk = be.read(want, fmt)
    assert rpk.write(fmt, SEL, len(SELECTORS)) == want
    assert rpk.usable_rows == gpk.usable_rows and rpk.proof_size == gpk.proof_size
    proof = be.prove(gpk)
    assert len(proof) == gpk.proof_size
    assert be.prove(rpk) == proof
    rpk.close()
    gpk.close()
    be.close()


def _be32_at(data, off, value):
    return data[:off] + struct.pack(">I", value) + data[off + 4:]


def test_every_rejection_keeps_its_code_and_text(ctx, monkeypatch):
    """Each bad description or stream raises CqError -1 with the text of the check it trips; afterwards the same context and
    params still build a key that proves to the same bytes, and the objects close in either order."""
    from sha2_on_cq_halo2_amd import CqError, ParamsKZG, StaticTable
    from sha2_on_cq_halo2_amd import proving_key as api  # the module `ProvingKey` resolves `_lower_plonk` in

    fx = _env("lookup")
    be = _Backend(ctx, fx)
    first = be.create()
    proof = be.prove(first)
    raw = first.to_bytes(SEL, len(SELECTORS))
    assert raw == fx["raw"]
    circuit = fx["circuit"]
    nfix, nperm, ext = circuit.num_fixed, fx["nperm"], len(fx["pk"].l0)

    def rejected(text, build):
        with pytest.raises(CqError) as e:
            build()
        assert e.value.code == -1 and text in str(e.value), (text, str(e.value))

    def tampered(tamper):
        """be.create() with `tamper` applied to the cq_plonk the API lowered"""
        real = api._lower_plonk

        def lowered(*a, **kw):
            pl = real(*a, **kw)
            tamper(pl)
            return pl

        monkeypatch.setattr(api, "_lower_plonk", lowered)
        try:
            return be.create()
        finally:
            monkeypatch.setattr(api, "_lower_plonk", real)

    # ---- descriptions
    other = ParamsKZG.setup_from_toxic_waste(ctx, K + 1, be.sm)
    rejected("pk: circuit k differs from params k", lambda: be.create(params=other))
    other.close()
    big = StaticTable.setup_from_toxic_waste(ctx, B.to_mont_limbs(TABLE + [100 + i for i in range(16)]), be.sm)
    good_tables = be.tables
    be.tables = {"t": big}
    be.cs = to_backend_cs(circuit, be.tables)
    rejected("pk: table size differs from the table config", be.create)
    be.tables = good_tables
    be.cs = to_backend_cs(circuit, be.tables)
    big.close()
    rejected("pk: static lookups need a table config and b0_g1_bound", lambda: be.create(cfg=None))
    rejected("pk: static lookups need a table config and b0_g1_bound", lambda: be.create(b0=None))

    def set_word(field, index, value):
        def tamper(pl):
            getattr(pl, field)[index] = value
        return tamper

    rejected("pk: advice query column out of range", lambda: tampered(set_word("advice_query_columns", 0, circuit.num_advice)))
    rejected("pk: fixed query column out of range", lambda: tampered(set_word("fixed_query_columns", 0, nfix)))
    rejected("pk: permutation column out of range", lambda: tampered(set_word("perm_column_indices", 0, circuit.num_advice)))
    mapping = np.array(fx["mapping"], dtype=np.uint32)
    for cell, entry in (((1, 7), (0, N_ROWS)), ((nperm - 1, N_ROWS - 1), (nperm, 0))):
        bad = mapping.copy()
        bad[cell] = entry
        rejected("pk: permutation mapping out of range", lambda: be.create(permutation=bad))

    def few_rows(pl):
        pl.blinding_factors = N_ROWS - 2  # n < bf + 3

    rejected("pk: not enough rows available", lambda: tampered(few_rows))
    rejected("gate program: unknown opcode", lambda: tampered(set_word("gate_programs", 0, 0xEE)))
    # ---- streams, in every format: header, polynomial length, slice count, length of the whole
    processed = SM.pk_raw_to_processed(raw, nperm, len(SELECTORS))
    for fmt, data, point in ((RAW, raw, 64), (RAW_UNCHECKED, raw, 64), (PROCESSED, processed, 32)):
        l0_len = 8 + point * (nfix + nperm) + len(SEL)
        fixed_count = l0_len + 3 * (4 + 32 * ext)
        assert struct.unpack(">I", data[l0_len:l0_len + 4])[0] == ext and struct.unpack(">I", data[fixed_count:fixed_count + 4])[0] == nfix
        rejected("pk: serialized key does not match the circuit", lambda: be.read(_be32_at(data, 0, K + 1), fmt))
        rejected("pk: serialized key does not match the circuit", lambda: be.read(_be32_at(data, 4, nfix + 1), fmt))
        rejected("pk: serialized polynomial has the wrong length", lambda: be.read(_be32_at(data, l0_len, ext - 1), fmt))
        rejected("pk: serialized key has a different number of polynomials", lambda: be.read(_be32_at(data, fixed_count, nfix - 1), fmt))
        rejected("pk: trailing bytes after the serialized key", lambda: be.read(data + bytes(5), fmt))
        rejected("pk: serialized polynomial has the wrong length", lambda: be.read(data[:-5], fmt))
    rejected("pk: unknown serde format", lambda: be.read(raw, 7))
    # ---- the context, the params and the tables are as good as before
    again = be.create()
    assert be.prove(again) == proof
    first.close()      # a key before the objects it was built on ...
    be.params.close()
    be.cfg.close()
    again.close()      # ... and one after them: the last key frees them
    for t in be.tables.values():
        t.close()


def test_retabling_for_two_ranks_and_back(ctx):
    """cq_pk_set_sharding(rank 0 of 2) rebuilds the key's window tables for the rank's slices (the all-gather callback
    would hand back the rank's own part alone; no proof is taken while sharded), world 1 brings the whole-array tables
    back: the proof is the unsharded one.  (Two real ranks prove in tests/test_parallel_gpu.py.)"""
    from sha2_on_cq_halo2_amd import api

    be = _Backend(ctx, _env("lookup"))
    gpk = be.create()
    proof = be.prove(gpk)

    def own_part_only(_user, send, recv, nbytes):
        C.memmove(recv, send, nbytes)
        return 0

    cb = api._ALLGATHER_T(own_part_only)
    ctx._chk(ctx.lib.cq_pk_set_sharding(gpk.h, 0, 2, C.cast(cb, C.c_void_p), None))
    gpk.set_sharding(0, 1)
    assert be.prove(gpk) == proof
    gpk.close()
    be.close()

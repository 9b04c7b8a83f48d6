"""SHA-256 of messages of variable length with constrained padding: one key built for `max_blocks` proves
SHA-256(m) = digest for any byte string m of 0 .. 64 * max_blocks - 9 bytes, several messages in one proof (DESIGN.md,
"Variable-length messages").

The segments are those of sha256_segments.batch -- one chain of max_blocks blocks per message, every word private -- under
the variable-length variant of the constraint system (sha256_circuit._constraint_system(..., varlen=True)): the gates force
the words up to the FINAL block -- the first with room for 0x80 and the 64-bit length -- to be pad(m) for the L-byte m they
spell, and the public digest to be the chaining value behind that block.  L is private unless `public_length`.  The
witness is synthesised from the raw bytes on the GPU by `cq_sha256_synthesize_varlen_dev`.

`continued`: the chain starts from a public chaining value H_in after a public number of bytes `base` instead of the IV
after none (DESIGN.md "Wired initial states"); the witness comes from `cq_sha256_synthesize_varlen_from_dev`.
"""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np

from . import sha256_circuit as SC
from . import sha256_segments as SS
from .context import Context

VAR = SC.VAR
MIN_TABLE_BITS = VAR["MIN_TABLE_BITS"]
MAX_TOTAL_BYTES = 1 << 29  # the bit length of base + message is one 32-bit word: word 14 of the final block is forced to zero


def check_base(base: int, max_blocks: int):
    """What a verifier must check of a continued proof's public `base`, which the circuit does not range-check: a multiple
    of 64 with base + 64 * max_blocks <= 2^29.  ValueError otherwise."""
    if base < 0 or base % 64:
        raise ValueError(f"a base of {base} bytes is no multiple of 64")
    if base + 64 * max_blocks > MAX_TOTAL_BYTES:
        raise ValueError(f"a base of {base} bytes and {max_blocks} blocks reach past 2^29 bytes")


def max_length(max_blocks: int) -> int:
    """The longest message, in bytes, whose padding fits max_blocks blocks."""
    return 64 * max_blocks - 9


def region_row(first_region: int, block: int, region: int) -> int:
    """Row 0 of region `region` (0 .. 67; 68 .. 71 of the last block: the tail) of block `block` of the segment that starts
    at `first_region`."""
    return SC.REGION_ROWS * (first_region + SC.BLOCK_REGIONS * block + region)


def describe(k: int, max_blocks_list, table_bits: int = 12, public_length: bool = False, dense="dense", spread="spread",
             continued: bool = False) -> SC.Description:
    """The variable-length constraint system with the fixed columns and copies of one segment per message; `blocks` is the
    tuple of the segments' block counts.  Instance: rows 8j .. 8j + 7 the digest of message j; with `public_length` the
    lengths, one row per message, behind all the digests.  With `continued`, behind those, 9 rows per message: H_in[0..7],
    the state the message's first block starts from, and `base`, the bytes absorbed before it; the eight state cells of
    block 0 are copied from them instead of from `const`, and so is the carry-in length of block 0, so every length counts
    from `base` and a public length is the total.  ValueError for table_bits outside [12, 16] or segments that do
    not fit 2^k rows."""
    if not MIN_TABLE_BITS <= table_bits <= SC.MAX_TABLE_BITS:
        raise ValueError(f"table_bits must be in [{MIN_TABLE_BITS}, {SC.MAX_TABLE_BITS}]: a boundary word's bytes are cut in 12-bit halves")
    max_blocks_list = tuple(int(b) for b in max_blocks_list)
    if not max_blocks_list or min(max_blocks_list) < 1:
        raise ValueError("at least one message, each of at least one block")
    plan = SS.batch(max_blocks_list)
    names = SC.FIXED_VARLEN
    cs, adv, fcol, inst, cells, word = SC._constraint_system(table_bits, dense, spread, varlen=True)
    n, X, Y, const = 1 << k, adv[2 * SC.PAIRS], adv[2 * SC.PAIRS + 1], fcol["const"]
    count = len(max_blocks_list)
    first_from = (9 if public_length else 8) * count  # the first instance row of the states and bases
    rows, usable, instance_rows = SS.rows_for(plan), n - (cs.blinding_factors() + 1), first_from + (9 * count if continued else 0)
    if max(rows, instance_rows) > usable:
        raise ValueError(f"{count} segments need {rows} rows and {instance_rows} instance rows, 2^{k} has {usable} usable")
    fixed = {name: np.zeros(n, dtype=np.uint64) for name in names}
    copies = []
    arow, erow = (word[(SC.SRC[s], SC.FORM_WORD)].row for s in "AE")
    M, LEN = VAR["ROW_M"], VAR["ROW_LEN"]
    IN, FLAG, VALUE, OUT = (VAR["ROW_" + s] for s in ("IN", "FLAG", "VALUE", "OUT"))
    data_scale = f"scale{VAR['SLOT_DATA']}"

    def from_const(value, row):  # a Y cell pinned to a constant through `const` on the same row
        fixed["const"][row] = value
        copies.append(((const, row), (Y, row)))

    for j, (first, blocks) in enumerate(zip(SS.first_regions(plan), max_blocks_list)):
        SC._assign_segment(fixed, copies, first, blocks, None, table_bits, adv, fcol, inst, cells, word, [None] * 8 if continued else None)
        for w in range(8 if continued else 0):  # state word w: region 3 - w % 4 of block 0, A row for w < 4, else E row
            copies.append(((inst, first_from + 9 * j + w), (X, region_row(first, 0, 3 - w % 4) + (arow if w < 4 else erow))))
        for i in range(blocks):
            at = lambda region, block=i: region_row(first, block, region)
            words = [at(4 + t) for t in range(16)]
            before = [at(4 + t, i - 1) for t in range(16)] if i else None
            for base in words:
                fixed["q_vpad" if base != words[15] else "q_vlength"][base] = 1
                fixed[data_scale][base: base + 2] = 1 << (table_bits - 12)
            if i == blocks - 1:
                fixed["q_vlast"][words[13]] = 1
            # the carry-in region: (m, len) the block starts from -- (1, 0), or word 15's of the block before, the length
            # times that block's m_13
            carry = at(VAR["REGION_CARRY"])
            if i == 0:
                from_const(1, carry + M)
                if continued:
                    copies.append(((inst, first_from + 9 * j + 8), (Y, carry + LEN)))
                else:
                    from_const(0, carry + LEN)
            else:
                fixed["q_vcarry"][carry] = 1
                copies.append(((Y, before[15] + M), (Y, carry + M)))
                copies.append(((Y, before[15] + LEN), (Y, carry + VALUE)))
                copies.append(((Y, before[13] + M), (Y, carry + OUT)))
            # the final flag: m_13 of the block before (1 for the first block) minus m_13 of this block
            final = at(VAR["REGION_FINAL"])
            fixed["q_vfinal"][final] = 1
            if i == 0:
                from_const(1, final + IN)
            else:
                copies.append(((Y, before[13] + M), (Y, final + IN)))
            copies.append(((Y, words[13] + M), (Y, final + FLAG)))
            # the sums: digest word w (and the length) selected so far + flag * the value behind this block; the chaining
            # value stands in the state regions of the next block, or in the tail
            for w in range(9):
                region = VAR["REGION_SUM"] + w if w < 8 else VAR["REGION_LENGTH"]
                s = at(region)
                fixed["q_vsum"][s] = 1
                if i == 0:
                    from_const(0, s + IN)
                else:
                    copies.append(((Y, at(region, i - 1) + OUT), (Y, s + IN)))
                copies.append(((Y, final + VALUE), (Y, s + FLAG)))
                if w < 8:
                    copies.append(((X, at(SC.BLOCK_REGIONS + 3 - w % 4) + (arow if w < 4 else erow)), (Y, s + VALUE)))
                else:
                    copies.append(((Y, words[15] + LEN), (Y, s + VALUE)))
                if i == blocks - 1 and w < 8:
                    copies.append(((inst, 8 * j + w), (Y, s + OUT)))
                elif i == blocks - 1 and public_length:
                    copies.append(((inst, 8 * count + j), (Y, s + OUT)))
    return SC.Description(cs, adv, fcol, fixed, inst, copies, cells, table_bits, max_blocks_list, k, names)


class Sha256VarCircuit:
    """Proving key and GPU witness synthesis for SHA-256 of `len(max_blocks_list)` messages of variable length at 2^k
    rows: message j is any byte string of at most 64 * max_blocks_list[j] - 9 bytes.  The methods take the raw, unpadded
    messages; the padding is made on the device and forced by the circuit.  The digests are public; the lengths are too
    with `public_length` (instance rows behind all the digests), else private.

    `continued`: for each message the circuit proves "starting from the chaining value H_in after `base` bytes, absorbing m
    and the padding for a total length of base + len(m) gives this digest"; H_in and base are public (9 instance rows per
    message behind the others) and a public length is the total.  `base` is not range-checked by the circuit: the
    verifier checks it with `check_base`."""

    def __init__(self, ctx: Context, k: int, max_blocks_list, table_bits: int = 12, public_length: bool = False, setup: str = "toxic",
                 seed: int = 0x5348413243515F, continued: bool = False):
        self.max_blocks_list = tuple(int(b) for b in max_blocks_list)
        self.public_length, self.continued = public_length, continued
        SC._build_key(self, ctx, k, table_bits, setup, seed,
                      lambda dense, spread: describe(k, self.max_blocks_list, table_bits, public_length, dense, spread, continued))
        self._states = ctx.alloc(32 * len(self.max_blocks_list)) if continued else None
        self._states_ptr = self._bases = self.states = self.bases = None
        self.rows = sum(SC.rows_for(b) for b in self.max_blocks_list)
        self._seg_blocks = np.array(self.max_blocks_list, dtype=np.uint32)
        self._bytes_len = sum(max_length(b) for b in self.max_blocks_list)
        self._bytes = ctx.alloc(self._bytes_len)
        self._digests = ctx.alloc(32 * len(self.max_blocks_list))
        self._offsets = self._lens = None
        self.digest_words = self.lengths = self.instances = None

    # ---- witness ----
    def _call(self, arr):
        """The entry point alone, on the bytes, offsets and lengths of the last upload."""
        ctx = self.ctx
        if self.continued:
            ctx._chk(ctx.lib.cq_sha256_synthesize_varlen_from_dev(ctx.h, self.table_bits, self._seg_blocks.ctypes.data, len(self._seg_blocks),
                                                                  self._bytes.ptr, self._bytes_len, self._offsets.ctypes.data,
                                                                  self._lens.ctypes.data, self._states_ptr, self._bases.ctypes.data, self.n, arr,
                                                                  self._digests.ptr))
            return
        ctx._chk(ctx.lib.cq_sha256_synthesize_varlen_dev(ctx.h, self.table_bits, self._seg_blocks.ctypes.data, len(self._seg_blocks),
                                                         self._bytes.ptr, self._bytes_len, self._offsets.ctypes.data,
                                                         self._lens.ctypes.data, self.n, arr, self._digests.ptr))

    def synthesize(self, messages, states=None, bases=None, states_ptr=None):
        """Uploads the raw bytes, pads them and fills the advice columns on the GPU (cq_sha256_synthesize_varlen_dev) and
        downloads the digests; returns (device columns, instances).  ValueError, before anything is launched, for a
        message longer than its segment holds.  A continued circuit also takes `states`, per message the 8 words of H_in,
        and `bases`, per message the bytes absorbed before it; with `states_ptr` the states are on the device already
        (8 words per message) and `states` is the host's copy for the instance."""
        messages = [bytes(m) for m in messages]
        if self.continued:
            if states is None or bases is None or len(states) != len(messages) or len(bases) != len(messages) or any(len(h) != 8 for h in states):
                raise ValueError("a continued circuit takes a state of 8 words and a base per message")
            for base, b in zip(bases, self.max_blocks_list):
                check_base(int(base), b)
            self.states, self.bases = [[int(x) for x in h] for h in states], [int(b) for b in bases]
            self._bases = np.array(self.bases, dtype=np.uint64)
            self._states_ptr = states_ptr or self._states.upload(np.array(self.states, dtype=np.uint32)).ptr
        elif states is not None or bases is not None or states_ptr is not None:
            raise ValueError("states and bases: only for a continued circuit")
        if len(messages) != len(self.max_blocks_list):
            raise ValueError(f"{len(self.max_blocks_list)} messages, not {len(messages)}")
        for j, (m, b) in enumerate(zip(messages, self.max_blocks_list)):
            if len(m) > max_length(b):
                raise ValueError(f"message {j}: {len(m)} bytes, {b} blocks hold at most {max_length(b)}")
        lens = np.array([len(m) for m in messages], dtype=np.uint64)
        self._lens, self._offsets = lens, np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        data = np.frombuffer(b"".join(messages), dtype=np.uint8)
        if len(data):
            self._bytes.upload(data)
        self._call((C.c_void_p * SC.ADVICE_COLUMNS)(*[c.ptr for c in self.cols]))
        self.digest_words = self._digests.download((len(messages), 8), np.uint32).tolist()
        self.lengths = [len(m) for m in messages]
        totals = [n_ + b for n_, b in zip(self.lengths, self.bases)] if self.continued else self.lengths
        public = [x for d in self.digest_words for x in d] + (totals if self.public_length else [])
        if self.continued:
            public += [x for h, b in zip(self.states, self.bases) for x in h + [b]]
        self.instance_words = public
        self.instances = [SS._words_to_mont(public)]
        return self.cols, self.instances

    @property
    def digests(self):
        """The digests of the last synthesis, 32 big-endian bytes each, in message order."""
        return [struct.pack(">8I", *d) for d in self.digest_words]

    def check_witness(self, messages, max_failures: int = 64, **from_):
        cols, inst = self.synthesize(messages, **from_)
        return self.pk.check_witness([c.ptr for c in cols], instances=inst, max_failures=max_failures)

    def assert_satisfied(self, messages, **from_):
        cols, inst = self.synthesize(messages, **from_)
        self.pk.assert_satisfied([c.ptr for c in cols], instances=inst)

    def create_proof(self, messages, seed: int = 1, **from_):
        """(proof bytes, digests): create_proof with the digest words -- and the lengths, if public; the states and bases, if
        continued -- as the public inputs."""
        cols, inst = self.synthesize(messages, **from_)
        return self.pk.create_proof_dev([c.ptr for c in cols], seed=seed, instances=inst), self.digests

    check, prove = check_witness, create_proof  # the names Sha256SegmentsCircuit uses

    def close(self):
        for o in (self._bytes, self._digests) + ((self._states,) if self._states is not None else ()):
            o.close()
        SC._close_key(self)

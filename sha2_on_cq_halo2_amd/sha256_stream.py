"""SHA-256 of one long message over a sequence of proofs under two keys (DESIGN.md "Wired initial states").

The message is cut into body pieces of exactly 64 * body_blocks bytes and a tail.  Every body piece is proved by one
`Sha256MidstateCircuit`: "these private blocks take the public H_in to the public H_out".  The tail is proved by one
continued `Sha256VarCircuit` with a public length: "from the public H_in after the public `base` bytes, the tail and the
padding for base + len(tail) bytes give this digest".  A verifier checks every proof and then `link`s their instances:
the first H_in is the IV, every H_out is the next H_in, and `base` counts the body pieces.
"""
from __future__ import annotations

import struct

import numpy as np

from . import sha256_circuit as SC
from . import sha256_varlen as SV
from .context import Context
from .sha256_segments import Sha256MidstateCircuit


class Sha256Stream:
    """The two keys and the device buffer of a streamed hash.  `prove(message)` takes any byte string whose total length,
    rounded up to the tail's blocks, stays within 2^29 bytes."""

    def __init__(self, ctx: Context, k_body: int, body_blocks: int, k_tail: int, tail_max_blocks: int, **kw):
        self.ctx, self.body_blocks, self.tail_max_blocks = ctx, body_blocks, tail_max_blocks
        self.body = Sha256MidstateCircuit(ctx, k_body, body_blocks, **kw)
        self.tail = SV.Sha256VarCircuit(ctx, k_tail, [tail_max_blocks], public_length=True, continued=True, **kw)
        self._buf = None

    def pieces(self, length: int) -> int:
        """The number of body pieces of a message of `length` bytes: as many as leave a tail the tail circuit holds."""
        piece, room = 64 * self.body_blocks, SV.max_length(self.tail_max_blocks)
        return max(0, -(-(length - room) // piece))

    def prove(self, message: bytes, seed: int = 1):
        """[(proof bytes, instance words)]: one entry per body piece -- instance (H_out, H_in) -- and the tail's --
        (digest, total length, H_in, base).  The chaining values stay on the device from one synthesis to the next: the
        word buffer holds, per piece, its 8 state words and its message words, and a piece's digest is stored straight
        into the state words of the piece behind it (the tail's state behind the last)."""
        ctx, message = self.ctx, bytes(message)
        piece, count = 64 * self.body_blocks, self.pieces(len(message))
        SV.check_base(piece * count, self.tail_max_blocks)
        stride = 8 + 16 * self.body_blocks  # words per piece
        host = np.zeros(stride * count + 8, dtype=np.uint32)
        host[:8] = SC.IV256
        for p in range(count):
            host[stride * p + 8: stride * (p + 1)] = struct.unpack(f">{16 * self.body_blocks}I", message[piece * p: piece * (p + 1)])
        if self._buf is None or self._buf.nbytes < host.nbytes:
            if self._buf is not None:
                self._buf.close()
            self._buf = ctx.alloc(host.nbytes)
        self._buf.upload(host)
        out, state = [], list(SC.IV256)
        for p in range(count):
            at = self._buf.ptr + 4 * stride * p
            cols, inst = self.body.synthesize_dev(at, at + 4 * stride, state)
            out.append((self.body.pk.create_proof_dev([c.ptr for c in cols], seed=seed + p, instances=inst), list(self.body.instance_words)))
            state = self.body.h_out
        cols, inst = self.tail.synthesize([message[piece * count:]], states=[state], bases=[piece * count],
                                          states_ptr=self._buf.ptr + 4 * stride * count)
        out.append((self.tail.pk.create_proof_dev([c.ptr for c in cols], seed=seed + count, instances=inst), list(self.tail.instance_words)))
        return out

    def close(self):
        if self._buf is not None:
            self._buf.close()
        self.body.close()
        self.tail.close()


def link(instances, body_blocks: int, tail_max_blocks: int | None = None):
    """What a verifier does with the instance words of a stream's proofs, each verified on its own, in order: every entry
    but the last is a body piece's 16 words (H_out, H_in), the last the tail's 18 (digest, total length, H_in, base).
    Checks that the first H_in is the IV, that every H_out is the next H_in, that `base` is 64 * body_blocks times the
    number of body pieces, and that it satisfies sha256_varlen.check_base -- with `tail_max_blocks` if given, else with the
    smallest tail, one block.  Returns (digest bytes, total length); ValueError names what does not hold."""
    instances = [[int(x) for x in inst] for inst in instances]
    if not instances or len(instances[-1]) != 18 or any(len(inst) != 16 for inst in instances[:-1]):
        raise ValueError("a stream is body instances of 16 words each and a tail instance of 18")
    *body, tail = instances
    digest, total, h_in, base = tail[:8], tail[8], tail[9:17], tail[17]
    state = list(SC.IV256)
    for p, inst in enumerate(body + [None]):
        got = h_in if inst is None else inst[8:]
        if got != state:
            raise ValueError(f"piece {p}: H_in is not " + ("the IV" if p == 0 else f"the H_out of piece {p - 1}"))
        state = inst[:8] if inst is not None else None
    if base != 64 * body_blocks * len(body):
        raise ValueError(f"the tail's base is {base}, {len(body)} pieces of {body_blocks} blocks are {64 * body_blocks * len(body)} bytes")
    SV.check_base(base, tail_max_blocks or 1)
    return struct.pack(">8I", *digest), total

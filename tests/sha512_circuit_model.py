"""Pure-Python model of the SHA-512 / SHA-384 compression circuit: tests/sha2_model.py at 64 bits -- integer cells from
FIPS 180-4 computed there (no library call but the layout table, which says where a bit field goes, not what it holds; the
round constants and initial hash values come from the primes' roots, not from the package), and its evaluator of the
constraint system's gates, static lookups and copy constraints over Python integers."""
import struct

from sha2_on_cq_halo2_amd import sha512_circuit as SC
from tests import sha2_model as M2
from tests.sha2_model import P, bitsum, evaluate, findings, spread  # noqa: F401

W = M2.W64
M64 = W.mask
K = W.K
IV = {SC.VARIANT_512: W.iv["sha512"], SC.VARIANT_384: W.iv["sha384"]}


def rotr(x, n):
    return M2.rotr(x, n, 64)


def region_words(message: bytes, blocks: int, variant: int = SC.VARIANT_512):
    """Per region of one message the dict of its 64-bit words by CQ_SHA256_SRC_* name, and the eight words of the final
    state."""
    regions, chaining = M2.compress(W, SC.pad(message, blocks), blocks, IV[variant])
    return M2.region_sources(W, regions), chaining[-1]


def witness(messages, blocks_list, variants, table_bits: int, n: int):
    """(18 advice columns of n integers, the instance words, the final state of every message): the messages' regions one
    behind another, zero behind the last."""
    cols = M2.columns(W, n)
    instance, states, first = [], [], 0
    for message, blocks, variant in zip(messages, blocks_list, variants):
        words, state = region_words(message, blocks, variant)
        M2.place(W, words, table_bits, cols, first * SC.REGION_ROWS)
        first += len(words)
        states.append(state)
        instance += state[:SC.DIGEST_WORDS[variant]]
    return cols, instance, states


def witness_one(message: bytes, blocks: int, table_bits: int, n: int, variant: int = SC.VARIANT_512):
    """(18 advice columns of n integers, the instance words) of a one-message circuit"""
    cols, instance, _ = witness([message], [blocks], [variant], table_bits, n)
    return cols, instance


def digest_bytes(state, variant: int = SC.VARIANT_512):
    count = SC.DIGEST_WORDS[variant]
    return struct.pack(f">{count}Q", *state[:count])

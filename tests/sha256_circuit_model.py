"""Pure-Python model of the SHA-256 compression circuit: tests/sha2_model.py at 32 bits -- integer cells from FIPS 180-4
computed there (no library call but the layout table, which says where a bit field goes, not what it holds; the round
constants and the initial hash value come from the primes' roots, not from the package), and its evaluator of the constraint
system's gates, static lookups and copy constraints over Python integers."""
import struct

from sha2_on_cq_halo2_amd import sha256_circuit as SC
from tests import sha2_model as M2
from tests.sha2_model import P, bitsum, evaluate, findings, spread  # noqa: F401

W = M2.W32
M32 = W.mask
K, IV = W.K, W.iv["sha256"]


def rotr(x, n):
    return M2.rotr(x, n, 32)


def region_words(message: bytes, blocks: int):
    """Per region the dict of its 32-bit words by CQ_SHA256_SRC_* name, and the digest words."""
    regions, chaining = M2.compress(W, SC.pad(message, blocks), blocks, IV)
    return M2.region_sources(W, regions), chaining[-1]


def witness(message: bytes, blocks: int, table_bits: int, n: int):
    """(18 advice columns of n integers, the 8 instance words)"""
    words, digest = region_words(message, blocks)
    cols = M2.columns(W, n)
    M2.place(W, words, table_bits, cols)
    return cols, digest


def digest_bytes(words):
    return struct.pack(">8I", *words)

"""GPU: SHA-512 / SHA-384 witness synthesis called directly on bare columns (no key), so that the chain kernel runs more
than one workgroup with lanes that differ in block count and variant, the expansion kernel many, two syntheses are queued
back to back, and the table width takes every count of non-empty chunks (6, 5, 4).  Every comparison is against the
pure-Python model, cell for cell over all 18 columns and all n rows, with n = rows + 5 (no multiple of 16 or 256: the rows
behind the last region come back zero) and the guard rows behind n untouched; every digest is compared with hashlib's."""
import hashlib
import random

import pytest

from sha2_on_cq_halo2_amd import sha512_circuit as SC
from sha2_on_cq_halo2_amd._lib import constants
from tests import sha512_circuit_model as M
from tests import sha512_direct as D

pytestmark = pytest.mark.gpu
ERR_ARG = constants()["CQ_ERR_ARG"]
HASH = {SC.VARIANT_512: hashlib.sha512, SC.VARIANT_384: hashlib.sha384}


def edgy_bytes(rng, length):
    """Bytes among which 0x00, 0x80 and 0xff are common: a pad byte in the wrong place next to them would show."""
    return bytes(rng.choice((0x00, 0x80, 0xFF)) if rng.random() < 0.5 else rng.randrange(256) for _ in range(length))


def blocks_of(length):
    return (length + 17 + 127) // 128


def big_case(seed):
    """(blocks, variants, messages): 70 one-block messages (among them 111 bytes of 0xff and of 0x00, the empty message
    and every length around the ends), two of two blocks (128 bytes of 0xff among them) and two of three (240 bytes of
    0x00 among them) in a fixed shuffled order, about a third of them SHA-384."""
    rng = random.Random(seed)
    lengths = [0, 1, 7, 8, 9, 110, 111, 111, 111] + [rng.randrange(112) for _ in range(61)] + [112, 128, 240, 367]
    messages = [edgy_bytes(rng, length) for length in lengths]
    messages[7], messages[8], messages[71], messages[72] = b"\xff" * 111, b"\x00" * 111, b"\xff" * 128, b"\x00" * 240
    order = list(range(len(messages)))
    rng.shuffle(order)
    messages = [messages[i] for i in order]
    variants = [SC.VARIANT_384 if rng.random() < 0.35 else SC.VARIANT_512 for _ in messages]
    return [blocks_of(len(m)) for m in messages], variants, messages


def padded_words(messages, blocks):
    return [w for m, b in zip(messages, blocks) for w in SC.pad(m, b)]


def digests_of(states, variants):
    return [M.digest_bytes(s, v) for s, v in zip(states, variants)]


class Case:
    """The messages and -- computed once, never changed -- the model's witness at n = rows + 5."""

    def __init__(self, blocks, variants, messages, table_bits=12):
        self.blocks, self.variants, self.messages, self.table_bits = blocks, variants, messages, table_bits
        self.words = padded_words(messages, blocks)
        self.rows = sum(SC.rows_for(b) for b in blocks)
        self.n = self.rows + 5
        self.want, _, self.states = M.witness(messages, blocks, variants, table_bits, self.n)

    def run(self, ctx, cols, check=True):
        rc, states = D.synthesize(ctx, cols, self.blocks, self.variants, self.words, self.n, self.table_bits)
        assert rc == 0
        if check:
            self.check(cols, states)
        return states

    def check(self, cols, states):
        cols.assert_equals(self.want, self.n)
        assert states == self.states
        assert digests_of(states, self.variants) == [HASH[v](m).digest() for m, v in zip(self.messages, self.variants)]
        # the rows behind the last region: zero in the model, so zero on the device
        assert all(col[r] == 0 for col in self.want for r in range(self.rows, self.n))


@pytest.fixture(scope="module")
def big():
    return Case(*big_case(5))


@pytest.fixture(scope="module")
def columns(ctx, big):
    cols = D.Columns(ctx, big.n)
    yield cols
    cols.close()


@pytest.fixture
def fresh(columns):
    columns.fill()
    return columns


def test_74_segments_in_one_call(ctx, big, fresh):
    assert len(big.blocks) == 74 and sorted(set(big.blocks)) == [1, 2, 3] and sum(big.blocks) == 80
    assert (74 + 63) // 64 == 2 and (big.n + 255) // 256 > 400 and big.n % 16 and big.n % 256  # chain and expansion workgroups
    assert set(big.blocks[:64]) == {1, 2, 3} and set(big.variants[:64]) == set(big.variants[64:]) == {SC.VARIANT_512, SC.VARIANT_384}
    words = set(big.words)
    assert 0 in words and (1 << 64) - 1 in words
    # the inputs reach every carry the layout holds but the largest of a_add's seven words
    cells = {name: next(c for c in SC.layout() if c.kind == SC.SRC[name]) for name in ("CARRY_A", "CARRY_E", "CARRY_W")}
    seen = {name: set(big.want[c.column][c.row:: SC.REGION_ROWS]) for name, c in cells.items()}
    assert seen["CARRY_A"] >= set(range(6)) and seen["CARRY_E"] == set(range(6)) and seen["CARRY_W"] == set(range(4))
    big.run(ctx, fresh)


def test_two_syntheses_queued_back_to_back(ctx, big, fresh):
    """Another witness of the same shape first, then the case on the same columns with nothing between them."""
    blocks, variants, messages = big_case(6)
    other_blocks = [blocks_of(len(m)) for m in messages]
    rc, first = D.synthesize(ctx, fresh, other_blocks, variants, padded_words(messages, other_blocks), big.n)
    assert rc == 0 and digests_of(first, variants) == [HASH[v](m).digest() for m, v in zip(messages, variants)]
    big.run(ctx, fresh)


@pytest.mark.parametrize("table_bits,chunks", [(11, 6), (13, 5), (16, 4)])
def test_every_count_of_non_empty_chunks(ctx, fresh, table_bits, chunks):
    """12 bits (6 chunks) is the big case's; here the widths at which a chunk starts at or above bit 64."""
    rng = random.Random(table_bits)
    messages = [b"\xff" * 111, edgy_bytes(rng, 200), b""]
    case = Case([1, 2, 1], [SC.VARIANT_512, SC.VARIANT_384, SC.VARIANT_384], messages, table_bits)
    assert sum(c * table_bits < 64 for c in range(SC.CHUNKS)) == chunks
    # a chunk past the word is zero in every region, the last chunk before it is not
    ev = sorted((c for c in SC.layout() if c.kind == SC.SRC["S0_EVEN"] and c.form == SC.FORM_PAIR), key=lambda c: c.per_table_bits)
    for c in ev:
        assert any(case.want[c.column][c.row:: SC.REGION_ROWS]) == (c.per_table_bits < chunks)
    case.run(ctx, fresh)


def test_bad_arguments_are_refused_and_nothing_is_written(ctx, fresh):
    blocks, variants = [1, 2], [SC.VARIANT_512, SC.VARIANT_384]
    words = padded_words([b"abc", b"\x01" * 150], blocks)
    rows = sum(SC.rows_for(b) for b in blocks)
    bad = [
        dict(table_bits=SC.MIN_TABLE_BITS - 1),
        dict(table_bits=SC.MAX_TABLE_BITS + 1),
        dict(blocks_list=[1, 0]),
        dict(variants=[SC.VARIANT_512, 2]),
        dict(n=rows - 1),
        dict(n=SC.rows_for(1)),
    ]
    for change in bad:
        args = dict(blocks_list=blocks, variants=variants, message_words=words, n=rows + 5, table_bits=12)
        args.update(change)
        rc, _ = D.synthesize(ctx, fresh, **args)
        assert rc == ERR_ARG, change
    fresh.assert_untouched()
    rc, states = D.synthesize(ctx, fresh, blocks, variants, words, rows)  # n = rows exactly is enough
    assert rc == 0 and digests_of(states, variants) == [hashlib.sha512(b"abc").digest(), hashlib.sha384(b"\x01" * 150).digest()]

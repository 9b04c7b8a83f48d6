"""CPU: the wired segments of both word widths are one piece of code (sha2_segments.py): the plans both widths have lower
to the same arrays, the source kinds are the same classes, and the word buffer refuses an out-of-range word at either
width.  Needs the built library's host entry points (the layout tables), no GPU."""
import numpy as np
import pytest

from sha2_on_cq_halo2_amd import sha2_segments as S
from sha2_on_cq_halo2_amd import sha256_segments as S256
from sha2_on_cq_halo2_amd import sha512_segments as S512
from sha2_on_cq_halo2_amd._lib import constants

PLANS = {
    "batch([1, 2])": (S256.batch([1, 2]), S512.batch([1, 2])),
    "double hash, 1 block": (S256.double_sha256(1), S512.double_sha512(1)),
    "merkle_tree(2)": (S256.merkle_tree(2), S512.merkle_tree(2)),
    "midstate(1)": (S256.midstate(1), S512.midstate(1)),
}


@pytest.mark.parametrize("name", sorted(PLANS))
def test_a_plan_both_widths_have_lowers_alike(name):
    narrow, wide = S256.lower(PLANS[name][0]), S512.lower(PLANS[name][1])
    for field in ("seg_blocks", "sources", "init_sources"):
        a, b = getattr(narrow, field), getattr(wide, field)
        assert a.dtype == b.dtype == np.uint32 and np.array_equal(a, b), field
    assert narrow.private_counts == wide.private_counts and narrow.words_len == wide.words_len
    assert narrow.consts.dtype == np.uint32 and wide.consts.dtype == np.uint64
    # the padding constants sort alike -- zero, the bit length, the 1 bit -- which is why equal sources read equal roles
    role = lambda bits, v: "zero" if v == 0 else "one bit" if v == 1 << (bits - 1) else v // bits  # a length: in words
    assert [role(32, v) for v in narrow.consts.tolist()] == [role(64, v) for v in wide.consts.tolist()]


def test_the_source_flags_are_equal_in_the_header():
    cq = constants()
    for flag in ("DIGEST", "IV"):
        assert cq["CQ_SHA256_SOURCE_" + flag] == cq["CQ_SHA512_SOURCE_" + flag] == getattr(S256, "SOURCE_" + flag) == getattr(S512, "SOURCE_" + flag)


def test_the_kinds_and_the_shared_functions_are_the_same_objects():
    for name in ("Private", "Const", "DigestWord", "Var", "Choice", "Xor", "Lowered", "PRIVATE", "word_buffer", "has_init", "shared_counts"):
        assert getattr(S256, name) is getattr(S512, name) is getattr(S, name), name
    assert issubclass(S256.Sha256SegmentsCircuit, S.Sha2SegmentsCircuit) and issubclass(S512.Sha512SegmentsCircuit, S.Sha2SegmentsCircuit)
    assert S256.PAD_64_BYTES == (S.Const(0x80000000),) + (S.Const(0),) * 14 + (S.Const(512),)
    assert S512.PAD_128_BYTES == (S.Const(1 << 63),) + (S.Const(0),) * 14 + (S.Const(1024),)


@pytest.mark.parametrize("module, top", [(S256, 1 << 32), (S512, 1 << 64)])
def test_the_word_buffer_refuses_a_word_out_of_range_at_either_width(module, top):
    var = module.Segment(1, (S.Var(0),) + (S.PRIVATE,) * 15)
    low = module.lower(module.Plan((var,), module.batch([1]).public))
    good = [list(range(15))]
    assert module.word_buffer(low, good, [top - 1]).tolist() == list(range(15)) + [top - 1]
    for values, shared in (([[top] + good[0][1:]], [0]), ([[-1] + good[0][1:]], [0]), (good, [top]), (good, [-1]), (good, []), ([good[0][:-1]], [0])):
        with pytest.raises(ValueError):
            module.word_buffer(low, values, shared)

"""CPU: segments that start from a wired state -- the plan types, their descriptions and lowering (no device), the
initial-state model against hashlib, and the verifier's `link` of a stream's instances."""
import hashlib
import struct

import numpy as np
import pytest

from sha2_on_cq_halo2_amd import sha256_circuit as SC
from sha2_on_cq_halo2_amd import sha256_segments as SS
from sha2_on_cq_halo2_amd import sha256_stream as ST
from sha2_on_cq_halo2_amd import sha256_varlen as SV
from tests import sha256_states_model as IM
from tests.sha2_model import words_of

P16 = (SS.PRIVATE,) * 16


# ---- 1. descriptions do not move ---------------------------------------------------------------------------------------------

def test_an_iv_init_is_the_description_without_one():
    src = P16 + SS.PAD_64_BYTES
    plans = [SS.Plan((SS.Segment(1, P16), seg), (1,)) for seg in
             (SS.Segment(2, src), SS.Segment(2, src, None), SS.Segment(2, src, tuple(SS.Const(v) for v in SC.IV256)))]
    descs = [SS.describe(11, p) for p in plans]
    for d in descs[1:]:
        assert d.copies == descs[0].copies and d.fixed_names == descs[0].fixed_names
        assert all(np.array_equal(d.fixed[name], descs[0].fixed[name]) for name in d.fixed_names)


def test_lower_without_an_init_is_all_sentinel():
    low = SS.lower(SS.double_sha256(2))
    assert low.init_sources.dtype == np.uint32 and low.init_sources.tolist() == [SS.SOURCE_IV] * 16 and SS.SOURCE_IV == 0xFFFFFFFF


def test_lower_orders_private_initial_words_before_the_message():
    plan = SS.Plan((SS.Segment(1, P16, (SS.PRIVATE, SS.Const(7), SS.Var(0)) + (SS.PRIVATE,) * 5),
                    SS.Segment(1, (SS.Const(7),) + P16[1:], tuple(SS.DigestWord(0, 7 - i) for i in range(8)))), (1,), (0,))
    low = SS.lower(plan)
    assert low.consts.tolist() == [7] and low.private_counts == [6 + 16, 15]
    assert low.init_sources[:8].tolist() == [1, 0, 1 + 22 + 15, 2, 3, 4, 5, 6]
    assert low.sources[:16].tolist() == list(range(7, 23)) and low.sources[16] == 0
    assert low.init_sources[8:].tolist() == [SS.SOURCE_DIGEST + 7 - i for i in range(8)]
    assert low.words_len == 1 + 22 + 15 + 1


def test_new_copies_stand_behind_the_old_ones():
    wired = tuple(SS.DigestWord(0, i) for i in range(6)) + (SS.Var(0), SS.PRIVATE)
    old = SS.Plan((SS.Segment(1, P16), SS.Segment(1, (SS.Var(0),) + P16[1:])), (1,))
    new = SS.Plan((old.segments[0], old.segments[1]._replace(init=wired)), (1,), (1,))
    d_old, d_new = SS.describe(11, old), SS.describe(11, new)
    # the IV's 8 const copies of segment 1 are gone; everything else keeps its order, the new copies follow
    gone = [c for c in d_old.copies if c not in d_new.copies]
    assert len(gone) == 8 and all(c[0][0] == d_old.fixed_columns["const"] for c in gone)
    kept = [c for c in d_old.copies if c in d_new.copies]
    assert d_new.copies[: len(kept)] == kept
    tail = d_new.copies[len(kept):]
    X, inst, first = d_new.advice[2 * SC.PAIRS], d_new.instance, SS.first_regions(new)[1]
    assert len(tail) == 6 + 1 + 8
    assert [c[1] for c in tail[:6]] == [(X, IM.state_row(first, i)) for i in range(6)]
    assert tail[6][1] == (X, IM.state_row(first, 6)) and tail[6][0][0] == X  # the var's message cell comes first
    assert tail[7:] == [((inst, 8 + i), (X, IM.state_row(first, i))) for i in range(8)]


@pytest.mark.parametrize("plan, names", [
    (SS.Plan((SS.Segment(1, P16), SS.Segment(1, P16, (SS.PRIVATE,) * 7 + (SS.Choice(0, SS.Var(0), SS.Var(1)),))), (0,)), ("segment 1", "initial word 7")),
    (SS.Plan((SS.Segment(1, P16, (SS.PRIVATE,) * 7),), (0,)), ("segment 0", "8 words")),
    (SS.Plan((SS.Segment(1, P16, (SS.PRIVATE,) * 3 + (SS.DigestWord(0, 0),) + (SS.PRIVATE,) * 4),), (0,)), ("segment 0", "initial word 3", "does not come before")),
    (SS.Plan((SS.Segment(1, P16), SS.Segment(1, P16, (SS.DigestWord(1, 0),) * 8)), (0,)), ("segment 1", "initial word 0")),
    (SS.Plan((SS.Segment(1, P16),), (0,), (0,)), ("public_init",)),
    (SS.Plan((SS.Segment(1, P16, (SS.PRIVATE,) * 8),), (0,), (0, 0)), ("public_init",)),
    (SS.Plan((SS.Segment(1, P16, (SS.PRIVATE,) * 8),), (0,), (1,)), ("public_init",)),
])
def test_check_plan_names_what_is_wrong(plan, names):
    with pytest.raises(ValueError) as e:
        SS.describe(11, plan)
    assert all(name in str(e.value) for name in names)


def test_builders():
    m = SS.midstate(2)
    assert m.public == (0,) and m.public_init == (0,) and m.segments[0].init == (SS.PRIVATE,) * 8 and m.segments[0].sources == (SS.PRIVATE,) * 32
    s = SS.sha224(1)
    assert [c.value for c in s.segments[0].init] == list(SS.IV224) and s.public == (0,) and s.public_init == ()
    d = SS.describe(10, s)
    assert sorted(int(v) for v in set(SS.IV224)) == sorted({int(d.fixed["const"][IM.state_row(0, i)]) for i in range(8)})


def test_continued_varlen_description():
    plain, cont = SV.describe(11, [1, 2], public_length=True), SV.describe(11, [1, 2], public_length=True, continued=True)
    inst, X, Y = cont.instance, cont.advice[2 * SC.PAIRS], cont.advice[2 * SC.PAIRS + 1]
    new = [c for c in cont.copies if c not in plain.copies]
    firsts = SS.first_regions(SS.batch([1, 2]))
    want = []
    for j, first in enumerate(firsts):
        want += [((inst, 18 + 9 * j + w), (X, IM.state_row(first, w))) for w in range(8)]
        want.append(((inst, 18 + 9 * j + 8), (Y, SV.region_row(first, 0, SC.VAR["REGION_CARRY"]) + SC.VAR["ROW_LEN"])))
    assert new == want and len(plain.copies) - len([c for c in plain.copies if c in cont.copies]) == 9 * 2
    assert SV.describe(11, [1, 2]).copies == SV.describe(11, [1, 2], continued=False).copies


# ---- 2. the model ------------------------------------------------------------------------------------------------------------

def test_the_model_split_at_every_block_boundary_is_hashlib():
    msg = bytes(range(150))  # pads to 3 blocks
    words = SC.pad(msg, 3)
    want = words_of(hashlib.sha256(msg).digest())
    for cut in range(4):
        mid = IM.compress(words[: 16 * cut], cut)[1][-1]
        assert IM.compress(words[16 * cut:], 3 - cut, mid)[1][-1] == want
    assert IM.compress(words, 3, SC.IV256)[1][-1] == want
    assert IM.varlen_cells(msg[128:], 1, 12, IM.state_after(msg[:128]), 128)[1] == want


def test_the_model_from_the_sha224_initial_value_is_hashlib():
    for msg in (b"", b"abc", bytes(range(100))):
        blocks = (len(msg) + 8) // 64 + 1
        digest = IM.compress(SC.pad(msg, blocks), blocks, SS.IV224)[1][-1]
        assert struct.pack(">8I", *digest)[:28] == hashlib.sha224(msg).digest()


# ---- 3. link -----------------------------------------------------------------------------------------------------------------

def stream_instances(message, body_blocks, tail_max_blocks):
    piece, room = 64 * body_blocks, 64 * tail_max_blocks - 9
    count = max(0, -(-(len(message) - room) // piece))
    state, out = list(SC.IV256), []
    for p in range(count):
        nxt = IM.state_after(message[piece * p: piece * (p + 1)], state)
        out.append(nxt + state)
        state = nxt
    tail = message[piece * count:]
    out.append(IM.varlen_cells(tail, tail_max_blocks, 12, state, piece * count)[1] + [len(message)] + state + [piece * count])
    return out


@pytest.mark.parametrize("length", [0, 100, 128, 128 + 183, 128 + 184, 3 * 128 + 5])
def test_link_accepts_a_consistent_chain(length):
    msg = bytes((7 * i + 3) % 256 for i in range(length))
    inst = stream_instances(msg, 2, 3)
    assert len(inst) == {0: 1, 100: 1, 128: 1, 311: 2, 312: 3, 389: 3}[length]
    assert ST.link(inst, 2, 3) == (hashlib.sha256(msg).digest(), length)
    assert ST.link(inst, 2) == (hashlib.sha256(msg).digest(), length)


def test_link_rejects_what_does_not_hold():
    msg = bytes(range(256)) * 2
    good = stream_instances(msg, 2, 3)
    assert len(good) == 4

    def broken(change):
        inst = [list(i) for i in good]
        change(inst)
        return inst

    def swap_base(value):
        return lambda inst: inst[-1].__setitem__(17, value)

    with pytest.raises(ValueError, match="piece 2: H_in is not the H_out of piece 1"):
        ST.link(broken(lambda inst: inst[1].__setitem__(3, inst[1][3] ^ 1)), 2, 3)
    with pytest.raises(ValueError, match="piece 3: H_in"):
        ST.link(broken(lambda inst: inst[-1].__setitem__(9, inst[-1][9] ^ 1)), 2, 3)
    with pytest.raises(ValueError, match="piece 0: H_in is not the IV"):
        ST.link(broken(lambda inst: inst[0].__setitem__(8, 0)), 2, 3)
    with pytest.raises(ValueError, match="piece 0: H_in is not the IV"):
        ST.link(good[1:], 2, 3)
    with pytest.raises(ValueError, match="base"):
        ST.link(broken(swap_base(3 * 128 + 64)), 2, 3)
    with pytest.raises(ValueError, match="base"):
        ST.link(good, 1, 3)
    # a base that breaks the bound: pieces so large that three of them reach 2^29 - 128, one step over for a 3-block tail
    big = ((1 << 29) - 128) // 64 // 3
    assert 64 * big * 3 + 64 * 3 > 1 << 29 and 64 * big * 3 + 64 <= 1 << 29
    with pytest.raises(ValueError, match="2\\^29"):
        ST.link(broken(swap_base(64 * big * 3)), big, 3)
    ST.link(broken(swap_base(64 * big * 3)), big)  # inside for the smallest tail
    with pytest.raises(ValueError, match="16 words"):
        ST.link(good[:-1], 2, 3)


def test_check_base():
    SV.check_base(0, 1), SV.check_base((1 << 29) - 64 * 3, 3)
    for base, blocks in ((32, 1), (-64, 1), ((1 << 29) - 64 * 3 + 64, 3)):
        with pytest.raises(ValueError):
            SV.check_base(base, blocks)

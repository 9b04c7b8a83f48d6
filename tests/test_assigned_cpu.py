"""CPU: the Python mirror of `Assigned<F>` (sha2_on_cq_halo2_amd.plonk.Assigned, AssignedColumn) against the independent
big-integer model tests/assigned_model.py, the field-homomorphism properties the reference's own proptests state
(plonk/assigned.rs, test module), and the host validator of the sparse row lists (csrc/assigned_host.hpp) run as a
stand-alone program under the host sanitizers."""
import itertools
import os
import shutil
import subprocess

import pytest

from oracle import bn254 as B
from sha2_on_cq_halo2_amd.plonk import Assigned, AssignedColumn
from tests import assigned_model as M

P = B.R_MOD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pairs(seed=11, extra=40):
    """(model cell, mirror cell) pairs: the named edge cells, so that every pair of variants and every edge meets every
    other, and a seeded random tail."""
    rng = B.Xoshiro256ss(seed)
    f = lambda: B.fr_random(rng)
    cells = [M.Z, M.T(0), M.T(1), M.T(f()), M.T(P - 1), M.R(f(), 0), M.R(0, 0), M.R(0, f()), M.R(f(), 1), M.R(f(), f()),
             M.R(f(), P - 1), M.R(1, f())]
    for _ in range(extra):
        kind = rng.next_u64() % 3
        cells.append(M.Z if kind == 0 else M.T(f()) if kind == 1 else M.R(f(), f() if rng.next_u64() % 4 else 0))
    return [(c, _mirror(c)) for c in cells]


def _mirror(c):
    return Assigned.zero() if c[0] == "Z" else Assigned.trivial(c[1]) if c[0] == "T" else Assigned.rational(c[1], c[2])


def _same(model_cell, mirror_cell):
    """same variant, same numerator and denominator: the case analysis, not only the value"""
    kind = {"Z": Assigned.ZERO, "T": Assigned.TRIVIAL, "R": Assigned.RATIONAL}[model_cell[0]]
    if mirror_cell.kind != kind:
        return False
    if kind == Assigned.ZERO:
        return True
    return mirror_cell.num == model_cell[1] and (kind == Assigned.TRIVIAL or mirror_cell.den == model_cell[2])


def test_every_pair_of_variants_is_in_the_mix():
    kinds = {(a[0][0], b[0][0]) for a, b in itertools.product(_pairs(), repeat=2)}
    assert kinds == set(itertools.product("ZTR", repeat=2))


def test_unary_operations_match_the_model():
    for m, a in _pairs():
        assert _same(M.neg(m), -a) and _same(M.double(m), a.double()) and _same(M.square(m), a.square()), m
        assert _same(M.cube(m), a.cube()) and _same(M.invert(m), a.invert()), m
        assert a.evaluate() == M.evaluate(m) and a.is_zero_vartime() == M.is_zero(m), m
        assert a.numerator() == M.numerator(m) and a.denominator() == M.denominator(m), m


def test_binary_operations_match_the_model():
    ps = _pairs()
    for (m1, a1), (m2, a2) in itertools.product(ps, repeat=2):
        assert _same(M.add(m1, m2), a1 + a2), (m1, m2)
        assert _same(M.sub(m1, m2), a1 - a2), (m1, m2)
        assert _same(M.mul(m1, m2), a1 * a2), (m1, m2)
        assert (a1 == a2) == M.eq(m1, m2), (m1, m2)


def test_evaluate_is_a_field_homomorphism():
    """assigned.rs proptests: evaluating after an operation equals operating on the evaluations; invert maps 0 to 0."""
    ps = [a for _, a in _pairs(seed=12)]
    for a in ps:
        assert (-a).evaluate() == -a.evaluate() % P
        e = a.evaluate()
        assert a.invert().evaluate() == (pow(e, P - 2, P) if e else 0)
        assert a.double().evaluate() == 2 * e % P and a.square().evaluate() == e * e % P and a.cube().evaluate() == e * e * e % P
    for a, b in itertools.product(ps, repeat=2):
        ea, eb = a.evaluate(), b.evaluate()
        assert (a + b).evaluate() == (ea + eb) % P, (a, b)
        assert (a - b).evaluate() == (ea - eb) % P, (a, b)
        assert (a * b).evaluate() == ea * eb % P, (a, b)
        assert (a == b) == (ea == eb), (a, b)


def test_x_over_zero_rules():
    """assigned.rs:375-440: addition and subtraction with x/0 use zero, not the rules for fractions."""
    two, half, inv0 = Assigned.trivial(2), Assigned.rational(1, 2), Assigned.rational(1, 0)
    for a in (two, half):
        assert (a + inv0).evaluate() == a.evaluate() == (inv0 + a).evaluate()
        assert (inv0 - a).evaluate() == (-a).evaluate() and (a - inv0).evaluate() == a.evaluate()
    assert (two * inv0).evaluate() == 0 and inv0 == Assigned.zero() and inv0.is_zero_vartime()


def test_from_cells_round_trips_and_matches_the_model_arrays():
    n = 64
    ps = _pairs(seed=13)
    col = AssignedColumn.from_cells([a for _, a in ps], n)
    num, rows, den = M.to_arrays([m for m, _ in ps], n)
    assert B.from_mont_limbs(col.num) == num and list(col.den_rows) == rows and B.from_mont_limbs(col.den) == den
    assert col.n == n and all(int(r) < n for r in col.den_rows) and list(col.den_rows) == sorted(set(col.den_rows))
    back = col.cells()
    assert len(back) == n and all(c.kind == Assigned.ZERO for c in back[len(ps):])
    for (m, a), c in zip(ps, back):
        # a zero numerator on an unlisted row reads back as Zero: Trivial(0) and Zero are one cell in the format
        assert c.evaluate() == M.evaluate(m) and (c.kind == a.kind or (a.kind == Assigned.TRIVIAL and a.num == 0)), m
    again = AssignedColumn.from_cells(back, n)
    assert (again.num == col.num).all() and (again.den_rows == col.den_rows).all() and (again.den == col.den).all()
    # the model's batch inversion of the cells is the cell-by-cell evaluation
    assert M.batch_invert_assigned_ref([[m for m, _ in ps]]) == [[M.evaluate(m) for m, _ in ps]]


@pytest.fixture(scope="module")
def rows_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("assigned") / "assigned_rows")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "assigned_rows.cpp"), "-o", exe], check=True)

    def run(n, limit, rows):
        r = subprocess.run([exe, str(n), str(limit)] + [str(x) for x in rows], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        return tuple(int(x) for x in r.stdout.split())

    return run


def test_host_validator_under_the_sanitizers(rows_program):
    n = 2048
    # good lists: (count, entries below the limit)
    assert rows_program(n, 2000, []) == (0, 0)
    assert rows_program(n, 2000, [0]) == (1, 1)
    assert rows_program(n, 2000, [0, 5, 1999, 2000, 2047]) == (5, 3)
    assert rows_program(n, 0, [0, 1]) == (2, 0)
    assert rows_program(n, n, list(range(0, n, 3))) == (len(range(0, n, 3)),) * 2
    # unsorted, duplicate, out of range: the FIRST offending entry
    assert rows_program(n, n, [3, 9, 7, 8])[0] == 2
    assert rows_program(n, n, [3, 9, 9, 10])[0] == 2
    assert rows_program(n, n, [3, 9, n])[0] == 2
    assert rows_program(n, n, [n])[0] == 0
    assert rows_program(n, n, [4, 2, n, 1])[0] == 1
    assert rows_program(n, n, [0xFFFFFFFF])[0] == 0

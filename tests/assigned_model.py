"""Big-integer model of `Assigned<F>` (halo2_proofs/src/plonk/assigned.rs) and of `batch_invert_assigned_ref`
(poly.rs:174-210), written from the reference text and independent of sha2_on_cq_halo2_amd.plonk.Assigned.

A cell is a tuple: ("Z",), ("T", x) or ("R", num, den), values reduced mod r.  Every function follows the match arms of
the reference in their order."""
from oracle import bn254 as B

P = B.R_MOD
Z = ("Z",)


def T(x):
    return ("T", x % P)


def R(a, b):
    return ("R", a % P, b % P)


def is_zero(c):  # assigned.rs:299-308
    if c[0] == "Z":
        return True
    if c[0] == "T":
        return c[1] == 0
    return c[1] == 0 or c[2] == 0


def eq(a, b):  # assigned.rs:44-70
    if a[0] == "Z" and b[0] == "Z":
        return True
    if a[0] == "Z":
        return is_zero(b)
    if b[0] == "Z":
        return is_zero(a)
    if a[0] == "R" and a[2] == 0:
        return is_zero(b)
    if b[0] == "R" and b[2] == 0:
        return is_zero(a)
    if a[0] == "T" and b[0] == "T":
        return a[1] == b[1]
    if a[0] == "T":
        return a[1] * b[2] % P == b[1]
    if b[0] == "T":
        return b[1] * a[2] % P == a[1]
    return a[1] * b[2] % P == a[2] * b[1] % P


def neg(c):  # assigned.rs:74-83
    if c[0] == "Z":
        return Z
    if c[0] == "T":
        return T(-c[1])
    return R(-c[1], c[2])


def add(a, b):  # assigned.rs:92-122
    if a[0] == "Z":
        return b
    if b[0] == "Z":
        return a
    if a[0] == "R" and a[2] == 0:
        return b
    if b[0] == "R" and b[2] == 0:
        return a
    if a[0] == "T" and b[0] == "T":
        return T(a[1] + b[1])
    if a[0] == "R" and b[0] == "T":
        return R(a[1] + a[2] * b[1], a[2])
    if a[0] == "T" and b[0] == "R":
        return R(b[1] + b[2] * a[1], b[2])
    return R(a[1] * b[2] + a[2] * b[1], a[2] * b[2])


def sub(a, b):  # assigned.rs:171-176
    return add(a, neg(b))


def mul(a, b):  # assigned.rs:225-244
    if a[0] == "Z" or b[0] == "Z":
        return Z
    if a[0] == "T" and b[0] == "T":
        return T(a[1] * b[1])
    if a[0] == "R" and b[0] == "T":
        return R(a[1] * b[1], a[2])
    if a[0] == "T" and b[0] == "R":
        return R(b[1] * a[1], b[2])
    return R(a[1] * b[1], a[2] * b[2])


def double(c):  # assigned.rs:312-320
    if c[0] == "Z":
        return Z
    if c[0] == "T":
        return T(2 * c[1])
    return R(2 * c[1], c[2])


def square(c):  # assigned.rs:324-332
    if c[0] == "Z":
        return Z
    if c[0] == "T":
        return T(c[1] * c[1])
    return R(c[1] * c[1], c[2] * c[2])


def cube(c):  # assigned.rs:336-338
    return mul(square(c), c)


def invert(c):  # assigned.rs:341-347
    if c[0] == "Z":
        return Z
    if c[0] == "T":
        return R(1, c[1])
    return R(c[2], c[1])


def field_inv(x):
    """`Field::invert().unwrap_or(zero)`"""
    return pow(x, P - 2, P) if x % P else 0


def evaluate(c):  # assigned.rs:353-366
    if c[0] == "Z":
        return 0
    if c[0] == "T":
        return c[1]
    if c[2] == 1:
        return c[1]
    return c[1] * field_inv(c[2]) % P


def numerator(c):  # assigned.rs:281-287
    return 0 if c[0] == "Z" else c[1]


def denominator(c):  # assigned.rs:289-296
    return c[2] if c[0] == "R" else None


def batch_invert(values):
    """ff::BatchInvert (ff 0.12 batch.rs): Montgomery's trick, zeros skipped and left at zero."""
    acc, prefix = 1, []
    for v in values:
        prefix.append(acc)
        if v:
            acc = acc * v % P
    acc = field_inv(acc)
    out = list(values)
    for i in range(len(values) - 1, -1, -1):
        if values[i]:
            out[i] = acc * prefix[i] % P
            acc = acc * values[i] % P
    return out


def batch_invert_assigned_ref(columns):
    """poly.rs:174-210: `columns` = lists of cells of one length -> lists of field elements."""
    dens = [denominator(c) for col in columns for c in col]
    some = [i for i, d in enumerate(dens) if d is not None]
    for i, inv in zip(some, batch_invert([dens[i] for i in some])):
        dens[i] = inv
    out, at = [], 0
    for col in columns:
        out.append([numerator(c) * (1 if dens[at + r] is None else dens[at + r]) % P for r, c in enumerate(col)])
        at += len(col)
    return out


def to_arrays(cells, n):
    """The three arrays of cq_assigned_column as Python integers: (num[n], den_rows, den)."""
    num = [numerator(c) for c in cells] + [0] * (n - len(cells))
    rows = [r for r, c in enumerate(cells) if c[0] == "R"]
    return num, rows, [cells[r][2] for r in rows]

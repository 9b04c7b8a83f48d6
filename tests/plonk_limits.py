"""General-PLONK circuits that sit ON the limits key generation accepts (csrc/pk.hpp `pk_describe_plonk`, csrc/plonk.hpp):
constraint-system degree 3 .. 18, up to 64 permutation columns, gate programs of operand-stack depth up to 16, legacy
lookups up to 64 expressions wide, three phases -- and one step past each.  Same dict as `chain_circuit` /
`random_circuit` (tests/plonk_fixtures.py), so `oracle_env(k, builder=limit_circuit, ...)`, `to_backend_cs` and
tests/witness_check_model.py take them unchanged.  No GPU here."""
from oracle import bn254 as B
from oracle import cq_prover as CP
from oracle import plonk as PL

P = B.R_MOD
A, F, I = PL.ADVICE, PL.FIXED, PL.INSTANCE
MAX_ROTATIONS = 4  # distinct rotations per advice column, Rotation::cur() of `enable_equality` included


def far_rotations(k):
    """Rotations whose product with rot_scale (up to 32) leaves the extended domain several times over."""
    n = 1 << k
    return (-(n - 1), -(n // 2), n // 2, n - 1)


def program_stack_depth(words):
    """Largest operand-stack depth a compiled gate program (include/cq_halo2.h, CQ_GATE_*) reaches: the walk of
    `gate_program_check` (csrc/plonk.hip) over the same words."""
    from sha2_on_cq_halo2_amd import plonk as GP

    sp = deepest = pc = 0
    while pc < len(words):
        op = words[pc] & 0xFF
        pc += 1
        if op in (GP.GATE_ADVICE, GP.GATE_FIXED, GP.GATE_INSTANCE):
            pc += 1  # the rotation word
            sp += 1
        elif op in (GP.GATE_CONST, GP.GATE_CHALLENGE):
            sp += 1
        elif op in (GP.GATE_ADD, GP.GATE_MUL):
            sp -= 1
        else:
            assert op in (GP.GATE_NEG, GP.GATE_SCALE), op
        deepest = max(deepest, sp)
    assert sp == 1
    return deepest


def compiled_stack_depth(circuit, gate):
    """Depth of gate polynomial `gate` as the backend's `ConstraintSystem` mirror lowers it."""
    from tests.plonk_fixtures import to_backend_cs

    return program_stack_depth(to_backend_cs(circuit, {}).gates[gate].compile([]))


def permutation_sets(perm_columns, degree):
    return -(-perm_columns // (degree - 2))


def limit_circuit(k, degree, perm_columns, *, depth=None, rotations=(), legacy_width=0, phases=False, satisfied=False, seed=1):
    """Returns dict(circuit, fixed, advice, instances, mapping, tables) plus `gate_rows`: the rows on which every cell
    gate 0 reads is a usable one.

    Gate 0, degree exactly `degree`: q0 (a_0 - a_1) f_0 ... f_{degree-3}, the f_j advice, fixed and instance queries
    spread over all first-phase advice columns at `rotations` (default -1, 0, 1).
    Gate 1 (depth given): (x_0 + (x_1 + (... + x_{depth-1}))) q1 -- every x_i is on the operand stack before the first
    addition, and the selector is pushed once the sum is back to one slot, so the compiled program reaches exactly `depth`
    (asserted on the compiled words).  One leaf is scaled, one negated; with `phases` one is the challenge squeezed after
    the second phase, and the last leaf, the column `t`, is a third-phase column (the second-phase column is a leaf too).
    Permutation: exactly `perm_columns` columns, (A 0) (F) (I 0) (A) (F) (A) (A) (F) ..., about 20 copies, each column
    boundary of the product sets (a multiple of degree - 2) with a copy across it.  a_1 stays outside the permutation.
    Legacy lookup (legacy_width > 0): that many degree-1 input expressions, the table expressions equal to them.

    The key's side (fixed columns, mapping) does not depend on `satisfied`; fixed cells that share a copy cycle are equal.
    satisfied=False: random advice and instances.  satisfied=True: the cells of every copy cycle equalised, a_1 = a_0 on
    every usable row -- so q0 may be (and is) a random non-zero value on every usable row and zero on the blinding rows:
    with a random witness nearly every row then fails or is poisoned -- and t = -(the other leaves) on the rows of q1,
    which is 1 where every leaf reads usable rows and 0 elsewhere."""
    n = 1 << k
    rng = B.Xoshiro256ss(0x11A17 + seed)
    rnd = lambda m: rng.next_u64() % m
    rotations = tuple(rotations) or (-1, 0, 1)
    assert degree >= 3 and perm_columns >= 1 and (depth is not None or not phases)

    # ---- columns ----
    kinds = [I if i == 2 else F if i % 3 == 1 else A for i in range(perm_columns)]
    perm_advice, perm_fixed, num_instance = kinds.count(A), kinds.count(F), kinds.count(I)
    base_advice = max(perm_advice + 1, 3)  # a_1 is never a permutation column
    num_advice = base_advice + (1 if phases else 0) + (1 if depth is not None else 0)
    ph1 = base_advice if phases else None
    t_col = num_advice - 1 if depth is not None else None
    q0, q1 = 0, (1 if depth is not None else None)
    first_data_fixed = 1 + (1 if depth is not None else 0)
    num_data_fixed = max(perm_fixed, 1)
    num_fixed = first_data_fixed + num_data_fixed
    adv_perm_index = [0] + list(range(2, base_advice))  # advice columns of the permutation, in its order
    perm, na, nf = [], 0, 0
    for kind in kinds:
        if kind == A:
            perm.append((A, adv_perm_index[na]))
            na += 1
        elif kind == F:
            perm.append((F, first_data_fixed + nf))
            nf += 1
        else:
            perm.append((I, 0))

    # ---- queries: at most MAX_ROTATIONS distinct rotations per advice column ----
    used = {c: set() for c in range(num_advice)}
    for col in [idx for kind, idx in perm if kind == A] + [0, 1] + [c for c in (ph1, t_col) if c is not None]:
        used[col].add(0)  # read at Rotation::cur() below, whatever else reads them
    turn = [0]

    def adv_query(col, rot=None):
        if rot is None:
            rot = rotations[turn[0] % len(rotations)]
            turn[0] += 1
        if rot not in used[col] and len(used[col]) >= MAX_ROTATIONS:
            rot = sorted(used[col])[turn[0] % len(used[col])]
        used[col].add(rot)
        return PL.adv(col, rot)

    def data_fixed_query(j):
        return PL.fix(first_data_fixed + j % num_data_fixed, rotations[j % len(rotations)])

    # ---- gate 0 ----
    product = None
    for j in range(degree - 2):
        if j % 5 == 3:
            f = data_fixed_query(j)
        elif j % 5 == 4 and num_instance:
            f = PL.inst(0, rotations[j % len(rotations)] % 2)
        else:
            f = adv_query((2 + j) % base_advice)
        product = f if product is None else PL.mul(product, f)
    gate0 = PL.mul(PL.mul(PL.fix(q0), PL.sub(adv_query(0, 0), adv_query(1, 0))), product)
    gates = [gate0]

    # ---- gate 1 ----
    leaves = []
    if depth is not None:
        for i in range(depth - 1):
            if phases and i == 3:
                x = PL.chal(1)
            elif phases and i == 4:
                x = adv_query(ph1, 0)
            elif i % 4 == 3:
                x = data_fixed_query(i)
            else:
                x = adv_query(i % base_advice)
            if i == 1:
                x = PL.scale(x, 7)
            elif i == 2:
                x = PL.neg(x)
            leaves.append(x)
        leaves.append(adv_query(t_col, 0))
        nested = leaves[-1]
        for x in reversed(leaves[:-1]):
            nested = PL.add(x, nested)
        gates.append(PL.mul(nested, PL.fix(q1)))

    # ---- legacy lookup ----
    plookups = []
    if legacy_width:
        exprs = [PL.add(adv_query(i % base_advice), PL.scale(data_fixed_query(i), i + 1)) for i in range(legacy_width)]
        plookups = [(exprs, list(exprs))]

    advice_phases, challenge_phases = None, []
    if phases:
        advice_phases = [0] * num_advice
        advice_phases[ph1], advice_phases[t_col] = 1, 2
        challenge_phases = [0, 1]
    circuit = CP.CqCircuit(k, num_advice, [], num_fixed, num_instance, gates, perm, None, plookups, advice_phases, challenge_phases)
    assert circuit.degree() == degree, (circuit.degree(), degree)
    assert all(len(r) <= MAX_ROTATIONS for r in used.values())
    if depth is not None:
        assert compiled_stack_depth(circuit, 1) == depth
    bf = circuit.blinding_factors()
    u = n - (bf + 1)
    assert u >= 1, "no usable row"

    def rows_reading_usable_cells(gate):
        q = []
        PL.expr_queries(gate, q)
        rots = {r for kind, _, r in q if kind == A}
        return [r for r in range(u) if all((r + rot) % n < u for rot in rots)]

    gate_rows = rows_reading_usable_cells(gate0)

    # ---- cells ----
    fixed = [[B.fr_random(rng) for _ in range(n)] for _ in range(num_fixed)]
    fixed[q0] = [1 + rnd(1 << 60) if r < u else 0 for r in range(n)]
    if depth is not None:
        on = set(rows_reading_usable_cells(gates[1]))
        fixed[q1] = [1 if r in on else 0 for r in range(n)]
    adv = [[B.fr_random(rng) for _ in range(u)] for _ in range(num_advice)]
    instances = [[B.fr_random(rng) for _ in range(u)] for _ in range(num_instance)]

    # ---- copies: every set boundary crossed, every column kind met, then random pairs ----
    asm = PL.Assembly(n, perm)
    chunk = degree - 2
    pairs = [(b - 1, b) for b in range(chunk, perm_columns, chunk)]
    pairs = pairs[:: max(1, len(pairs) // 8)][:8]
    first = {kind: kinds.index(kind) for kind in (A, F, I) if kind in kinds}
    pairs += [(first[x], first[y]) for x in first for y in first if x < y]
    while len(pairs) < 20:
        pairs.append((rnd(perm_columns), rnd(perm_columns)))
    for lc, rc in pairs:
        asm.copy(perm[lc], rnd(u), perm[rc], rnd(u))

    # ---- copy cycles: fixed cells of one cycle agree (whatever the witness); a satisfied witness agrees with them ----
    def cell_ref(c, row):
        kind, idx = perm[c]
        return (fixed[idx] if kind == F else adv[idx] if kind == A else instances[idx]), row

    seen = set()
    for c in range(perm_columns):
        for row in range(n):
            if (c, row) in seen or asm.mapping[c][row] == (c, row):
                continue
            cycle, cur = [], (c, row)
            while cur not in seen:
                seen.add(cur)
                cycle.append(cur)
                cur = asm.mapping[cur[0]][cur[1]]
            in_key = [x for x in cycle if perm[x[0]][0] == F]
            lead = in_key[0] if in_key else cycle[0]
            col, r = cell_ref(*lead)
            value = col[r]
            for x in cycle:
                if perm[x[0]][0] == F or satisfied:
                    col, r = cell_ref(*x)
                    col[r] = value
    if satisfied:
        adv[1] = list(adv[0])

    # ---- later phases, and the column that closes gate 1 ----
    def t_values(ch, columns):
        """-(x_0 + ... + x_{depth-2}) on the rows of q1, the random draw elsewhere."""
        def get(kind, col, rot, row):
            src = columns[col] if kind == A else fixed[col] if kind == F else instances[col]
            r = (row + rot) % n
            return src[r] if r < len(src) else 0

        out = list(columns[t_col])
        for row in range(u):
            if fixed[q1][row]:
                out[row] = -sum(PL.expr_eval(x, lambda kind, col, rot: get(kind, col, rot, row), ch) for x in leaves[:-1]) % P
        return out

    if phases:
        a0, draw1, draw_t = list(adv[0]), list(adv[ph1]), list(adv[t_col])
        second = lambda ch: [(ch[0] * a0[r] + draw1[r]) % P for r in range(u)]
        adv[ph1] = second
        if satisfied:
            adv[t_col] = lambda ch: t_values(ch, [second(ch) if c_ == ph1 else draw_t if c_ == t_col else adv[c_] for c_ in range(num_advice)])
        else:
            adv[t_col] = lambda ch: [(draw_t[r] + ch[1]) % P for r in range(u)]
    elif depth is not None and satisfied:
        adv[t_col] = t_values((), adv)
    return dict(circuit=circuit, fixed=fixed, advice=adv, instances=instances, mapping=asm.mapping, tables={}, gate_rows=gate_rows)


# The shapes of tests/test_plonk_limits_gpu.py (and, for what the fixtures claim, of tests/test_plonk_limits_cpu.py):
# id -> (k, degree, permutation columns, builder keywords, openers)
def _cases():
    out = {}
    # every extended-domain factor, on both sides of each step: 2, 4, 4, 8, 8, 16, 16, 32; two full sets and a one-column set
    for d in (3, 4, 5, 6, 9, 10, 17, 18):
        out[f"deg{d}"] = (5, d, 2 * (d - 2) + 1, {}, ("gwc",))
    # the last set full, one column short, one column over (4 columns per set)
    for pc in (8, 7, 9):
        out[f"deg6-cols{pc}"] = (5, 6, pc, {}, ("gwc",))
    out["deg3-cols64"] = (5, 3, 64, {}, ("gwc", "shplonk"))  # 64 sets: mult[64], grid.y = 64, the z_{s-1} chain 63 deep
    out["deg18-cols64-k6"] = (6, 18, 64, {}, ("gwc", "shplonk"))  # 4 full sets of 16, extended domain 32n
    out["deg18-cols16"] = (5, 18, 16, {}, ("gwc",))  # one set holding all columns
    out["depth16-phases"] = (5, 4, 3, dict(depth=16, phases=True), ("gwc",))
    # far rotations times rot_scale; -(n-1) and the permutation's +1, -n/2 and n/2 are also one opening POINT each, which the
    # multi-open must group as the reference does (by point: csrc/pk.hpp `point_rotation`)
    for k in (5, 6):
        out[f"far-rotations-k{k}"] = (k, 6, 3, dict(rotations=far_rotations(k)), ("gwc",))
    for k in (7, 8):  # extended domain 256 (ext_pow_hi holds one entry) and 512 (the first use of ext_pow_hi[1])
        out[f"ext{2 << k}-k{k}"] = (k, 3, 5, {}, ("gwc",))
    out["smallest-k3"] = (3, 3, 2, {}, ("gwc",))  # n = 8 = blinding factors (5) + 3: two usable rows
    for w in (64, 3):
        out[f"legacy-width{w}"] = (5, 4, 3, dict(legacy_width=w), ("gwc",))
    return out


CASES = _cases()
# one step past each limit: id -> ((k, degree, permutation columns, builder keywords), the refusal's text)
REJECTED = {
    "degree19": ((5, 19, 3, {}), "pk: cs_degree out of range"),
    "cols65": ((5, 3, 65, {}), "pk: too many permutation columns"),
    "depth17": ((5, 4, 3, dict(depth=17)), "gate program: expression too deep for the operand stack"),
    "legacy-width65": ((5, 4, 3, dict(legacy_width=65)), "pk: legacy lookup width out of range"),
}

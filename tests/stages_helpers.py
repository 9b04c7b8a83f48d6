"""Helpers of tests/test_stages_gpu.py: a direct restatement of ProverGWC::create_proof (gwc/prover.rs:42-91) for arbitrary
queries through oracle.poly, and a transcript pair that records what crosses cq_multiopen_dev's callbacks."""
import numpy as np

from oracle import bn254 as B
from oracle import cq_prover as CP
from oracle.poly import eval_polynomial, kate_division, msm_affine

P = B.R_MOD


def gwc_prove(tr, n, queries, polys, g, commit=None):
    """queries: [(key, point, eval)] in order; polys: key -> coefficients (<= n); g: the SRS.  Per distinct point in
    first-seen order (gwc.rs:36-61): poly_batch = sum_i v^i p_i, eval_batch = sum_i v^i e_i over the point's queries
    (:62-78), the witness (poly_batch - eval_batch) / (X - point) (:80) and its commitment (:85).  commit(poly) replaces
    the MSM over g[: n - 1] (g may then be None): `trapdoor_commit` for large n, a scalar for the verifier identities."""
    if commit is None:
        commit = lambda w: msm_affine(w, g[: n - 1])
    v = tr.squeeze_challenge_scalar()
    points = []
    for _, pt, _ in queries:
        if pt not in points:
            points.append(pt)
    for pt in points:
        batch, eval_batch, pv = [0] * n, 0, 1
        for key, qpt, ev in queries:
            if qpt != pt:
                continue
            batch = [(a + pv * c) % P for a, c in zip(batch, list(polys[key]) + [0] * (n - len(polys[key])))]
            eval_batch = (eval_batch + pv * ev) % P
            pv = pv * v % P
        batch[0] = (batch[0] - eval_batch) % P
        w = kate_division(batch, pt)
        tr.write_point(commit(w))
    return v


class RecordingTranscript:
    """The oracle's Blake2bWrite behind cq_multiopen_dev's two callbacks (Montgomery limbs across the ABI)."""

    def __init__(self, fail_squeeze_at=None, fail_write_at=None):
        self.tr = CP.Blake2bWrite()
        self.tr.common_scalar(12345)
        self.challenges, self.points = [], []
        self.fail_squeeze_at, self.fail_write_at = fail_squeeze_at, fail_write_at

    def squeeze(self):
        if self.fail_squeeze_at == len(self.challenges):
            raise RuntimeError("squeeze refused")
        c = self.tr.squeeze_challenge_scalar()
        self.challenges.append(c)
        return B.to_mont_limbs([c])[0]

    def write(self, affine):
        if self.fail_write_at == len(self.points):
            raise RuntimeError("write refused")
        pt = B.points_from_mont_limbs(affine.reshape(1, 8))[0]
        self.points.append(pt)
        self.tr.write_point(pt)


class ScriptedTranscript:
    """No hash: hands out the given challenges in order and records what is written, so a test chooses y, v, u itself.
    Both faces: squeeze_challenge_scalar / write_point for the oracle's provers (ints and whatever their `commit`
    returns), squeeze / write for cq_multiopen_dev's callbacks (Montgomery limbs, as RecordingTranscript converts them)."""

    def __init__(self, challenges):
        self.script, self.challenges, self.points = list(challenges), [], []

    def squeeze_challenge_scalar(self):
        c = self.script[len(self.challenges)]  # an IndexError here fails the device call: more squeezes than scripted
        self.challenges.append(c)
        return c

    def write_point(self, pt):
        self.points.append(pt)

    def squeeze(self):
        return B.to_mont_limbs([self.squeeze_challenge_scalar()])[0]

    def write(self, affine):
        self.write_point(B.points_from_mont_limbs(affine.reshape(1, 8))[0])


def trapdoor_commit(s):
    """commit(p) = p(s) G: what the MSM over the powers [s^i]_1 of `setup_from_toxic_waste(k, s)` gives, in one scalar
    multiplication (tests/test_multiopen_shapes_cpu.py checks the two against each other once)."""
    return lambda poly: B.g1_mul(B.G1_GEN, eval_polynomial(poly, s))


def reference_transcript():
    tr = CP.Blake2bWrite()
    tr.common_scalar(12345)
    return tr


def evaluations(queries_kp, polys):
    return [(key, pt, eval_polynomial(polys[key], pt)) for key, pt in queries_kp]


class ComposedProver:
    """create_proof (plonk/prover.rs:51-779) for a single-phase circuit without legacy lookups or instance columns, driven
    stage by stage through the C ABI's device calls: the host keeps the transcript (the oracle's Blake2bWrite), the RNG
    stream (one cq_buffer_rng shared with the stage calls) and the order of the steps; everything O(n) is a library call.
    `seconds_in_library` adds up the wall time of those calls."""

    def __init__(self, ctx, gpk, fixed_host, mapping):
        import time

        from sha2_on_cq_halo2_amd import EvaluationDomain
        from sha2_on_cq_halo2_amd.api import domain_omega_int

        self.ctx, self.gpk, self.cs, self.lib, self.clock = ctx, gpk, gpk.cs, ctx.lib, time.perf_counter
        cs, k = gpk.cs, gpk.k
        self.k, self.n = k, 1 << k
        self.bf = cs.blinding_factors()
        self.u = self.n - (self.bf + 1)
        self.sets = -(-len(cs.permutation_columns) // (cs.degree() - 2))
        self.L = len(cs.static_lookups)
        self.dom = EvaluationDomain(ctx, cs.degree(), k)
        self.omega = domain_omega_int(k)
        self.seconds_in_library = 0.0
        n = self.n
        # the key's own polynomials, which the opening queries name: fixed columns and permutation polynomials
        self.fixed_polys = []
        for col in fixed_host:
            buf = ctx.to_device(col)
            self.dom.lagrange_to_coeff_dev(buf, buf)
            self.fixed_polys.append(buf)
        self.sigma_polys = []
        if len(cs.permutation_columns):
            pw = [1] * n
            for i in range(1, n):
                pw[i] = pw[i - 1] * self.omega % P
            dl = [pow(B.FR_DELTA, c, P) for c in range(len(cs.permutation_columns))]
            for col in np.asarray(mapping):
                buf = ctx.to_device(B.to_mont_limbs([dl[int(c)] * pw[int(r)] % P for c, r in col]))
                self.dom.lagrange_to_coeff_dev(buf, buf)
                self.sigma_polys.append(buf)

    def _call(self, fn, *args):
        t0 = self.clock()
        self.ctx._chk(fn(*args))
        self.seconds_in_library += self.clock() - t0

    def _commit(self, fn, ptr, length):
        jac, aff = np.zeros(12, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
        self._call(fn, self.gpk.params.h, ptr, length, jac.ctypes.data)
        self._call(self.lib.cq_g1_to_affine, jac.ctypes.data, aff.ctypes.data)
        return B.points_from_mont_limbs(aff.reshape(1, 8))[0]

    def _eval(self, ptr, length, point):
        pt, out = B.to_mont_limbs([point])[0], np.zeros(4, dtype=np.uint64)
        self._call(self.lib.cq_eval_polynomial_dev, self.ctx.h, ptr, length, pt.ctypes.data, out.ctypes.data)
        return B.from_mont_limbs(out.reshape(1, 4))[0]

    def _rotate(self, x, rot):
        return x * pow(self.omega, rot % self.n, P) % P

    def prove(self, advice_bufs, rng_words, vk_repr, opener):
        """advice_bufs: DevBufs of n elements, rows below `u` assigned (the blinding rows are written here)."""
        ctx, gpk, cs, lib, n, u, bf, L, S = self.ctx, self.gpk, self.cs, self.lib, self.n, self.u, self.bf, self.L, self.sets
        words = np.ascontiguousarray(rng_words, dtype=np.uint64)
        rng = gpk._rng(rng_words=words)
        state = gpk._rng_keep[1]

        def draw(count):  # `count` x Fr::random from the shared stream
            w = [int(x_) for x_ in words[state.pos: state.pos + 8 * count]]
            state.pos += 8 * count
            return [B.from_u512(w[8 * i: 8 * i + 8], P) for i in range(count)]

        mont = lambda v: B.to_mont_limbs([v])[0]
        tr = CP.Blake2bWrite()
        tr.common_scalar(vk_repr)  # prover.rs:85
        # 1. advice: blinding rows, one unused blind per column, commit_lagrange (:346-374)
        A = len(advice_bufs)
        tails = [draw(bf + 1) for _ in range(A)]
        draw(A)
        for buf, tail in zip(advice_bufs, tails):
            t = B.to_mont_limbs(tail)
            self._call(lib.cq_dev_upload, ctx.h, buf.ptr + u * 32, t.ctypes.data, t.nbytes)
        for buf in advice_bufs:
            tr.write_point(self._commit(lib.cq_commit_lagrange_dev, buf.ptr, n))
        theta = tr.squeeze_challenge_scalar()  # :472
        adv_ptrs = [b_.ptr for b_ in advice_bufs]
        # 3. static_lookup::Argument::commit (:512-522)
        if L:
            t0 = self.clock()
            f, m, cm1 = gpk.cq_round1(adv_ptrs, mont(theta))
            self.seconds_in_library += self.clock() - t0
            for pt in B.points_from_mont_limbs(cm1.reshape(-1, 8)):
                tr.write_point(pt)
        beta = tr.squeeze_challenge_scalar()  # :529
        gamma = tr.squeeze_challenge_scalar()  # :532
        # 4. permutation::Argument::commit (:539-549), drawing on from the same stream
        z = None
        if S:
            t0 = self.clock()
            z, cmz = gpk.permutation_commit(adv_ptrs, mont(beta), mont(gamma), rng=rng)
            self.seconds_in_library += self.clock() - t0
            for pt in B.points_from_mont_limbs(cmz):
                tr.write_point(pt)
        # 6. commit_log_derivatives (:572-575), then vanishing::Argument::commit (vanishing/prover.rs:37-65)
        b = fc = None
        a0 = []
        if L:
            t0 = self.clock()
            b, fc, cm2, a0 = gpk.cq_round2(f, m, mont(theta), mont(beta))
            self.seconds_in_library += self.clock() - t0
            for pt in B.points_from_mont_limbs(cm2.reshape(-1, 8)):
                tr.write_point(pt)
        random_poly = ctx.to_device(B.to_mont_limbs(draw(n)))
        draw(1)
        tr.write_point(self._commit(lib.cq_commit_dev, random_poly.ptr, n))
        y = tr.squeeze_challenge_scalar()  # :584
        # 7. advice -> coefficients (:587-603), evaluate_h (:606-624), vanishing construct (vanishing/prover.rs:69-120)
        for buf in advice_bufs:
            t0 = self.clock()
            self.dom.lagrange_to_coeff_dev(buf, buf)
            self.seconds_in_library += self.clock() - t0
        ext = self.dom.extended_len
        t0 = self.clock()
        h = gpk.evaluate_h(adv_ptrs, mont(beta), mont(gamma), mont(theta), mont(y), ext, perm_z=z)
        none = ctx.alloc(32)
        h = gpk.cq_quotient(b or none, fc or none, mont(y), mont(beta), h_in=h, divide=True, ext=ext)
        self.dom.extended_to_coeff_dev(h, h)
        self.seconds_in_library += self.clock() - t0
        pieces = cs.degree() - 1
        draw(pieces)  # h_blinds (:95-98)
        for i in range(pieces):
            tr.write_point(self._commit(lib.cq_commit_dev, h.ptr + i * n * 32, n))
        x = tr.squeeze_challenge_scalar()  # :629
        xn = pow(x, n, P)
        # h(X) = sum_i x^(n i) h_i(X) (vanishing/prover.rs:131-135): one polynomial for the opening
        hp = B.from_mont_limbs(h.download((pieces * n, 4)))
        h_poly = [0] * n
        for i in reversed(range(pieces)):
            h_poly = [(a_ * xn + c_) % P for a_, c_ in zip(h_poly, hp[i * n:(i + 1) * n])]
        h_poly = ctx.to_device(B.to_mont_limbs(h_poly))
        # 8./9. the opening queries in the order ProverGWC receives them (:721-773), their evaluations in write order (:654-719)
        x_next, x_last = self._rotate(x, 1), self._rotate(x, -(bf + 1))
        q_adv = [(advice_bufs[c].ptr, n, self._rotate(x, r)) for c, r in cs.advice_queries]
        q_z = [(z.ptr + st * n * 32, n, pt) for st in range(S) for pt in (x, x_next)]
        q_zl = [(z.ptr + st * n * 32, n, x_last) for st in reversed(range(S - 1))]
        q_cq = [q for l in range(L) for q in ((b.ptr + (l * n + 1) * 32, n - 1, x), (fc.ptr + l * n * 32, n, x))]
        q_fix = [(self.fixed_polys[c].ptr, n, self._rotate(x, r)) for c, r in cs.fixed_queries]
        q_sig = [(p_.ptr, n, x) for p_ in self.sigma_polys]
        q_rnd = (random_poly.ptr, n, x)
        ev = lambda q: self._eval(*q)
        for q in q_adv + q_fix + [q_rnd] + q_sig:
            tr.write_scalar(ev(q))
        for st in range(S):  # permutation/prover.rs:243-290
            tr.write_scalar(ev(q_z[2 * st]))
            tr.write_scalar(ev(q_z[2 * st + 1]))
            if st + 1 < S:
                tr.write_scalar(ev((z.ptr + st * n * 32, n, x_last)))
        for l in range(L):  # static_lookup/prover.rs:360-370
            tr.write_scalar(ev(q_cq[2 * l]))
            tr.write_scalar(ev(q_cq[2 * l + 1]))
            tr.write_scalar(B.from_mont_limbs(a0[l:l + 1])[0])
        queries = q_adv + q_z + q_zl + q_cq + q_fix + q_sig + [(h_poly.ptr, n, x), q_rnd]
        gpk.set_opener(opener)
        t0 = self.clock()
        gpk.multiopen([(p_, ln, mont(pt)) for p_, ln, pt in queries], lambda: mont(tr.squeeze_challenge_scalar()),
                      lambda aff: tr.write_point(B.points_from_mont_limbs(aff.reshape(1, 8))[0]))
        self.seconds_in_library += self.clock() - t0
        return bytes(tr.proof)

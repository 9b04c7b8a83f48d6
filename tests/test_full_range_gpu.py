"""Full-range inputs where the large-size tests mask them: the uniform inputs of the 2^18..2^20 NTTs, the table-mode MSM and
the large batch inversion keep word 3 below 2^60 (values < 2^252).  Here the same kernels take words over the whole range
below r, a block of r - 1 and a block whose lower eight 29-bit limbs are all 2^29 - 1 (tests/util.py full_range_words) --
the NTT and the batch inversion read these words directly as lazy limbs (field29.hpp)."""
import numpy as np
import pytest

from oracle import bn254 as B
from tests.util import full_range_words

pytestmark = pytest.mark.gpu


def _omega(log_n):
    w = B.FR_ROOT_OF_UNITY
    for _ in range(log_n, B.FR_S):
        w = w * w % B.R_MOD
    return w


@pytest.mark.parametrize("log_n", [18, 20])
def test_best_fft_full_range_inputs_match_c_oracle(ctx, log_n):
    from oracle import cbind as OC

    a = full_range_words(1 << log_n, 2000 + log_n)
    w = B.to_mont_limbs([_omega(log_n)])[0]
    assert np.array_equal(ctx.best_fft(a, w, log_n), OC.best_fft(a, w, log_n))


def test_msm_table_mode_k18_full_range_scalars_match_c_oracle(ctx):
    """A k = 18 table-mode batch (registered Lagrange SRS) over full-range scalar vectors, against `best_multiexp`'s C
    restatement."""
    from oracle import cbind as OC
    from sha2_on_cq_halo2_amd import ParamsKZG

    k = 18
    n = 1 << k
    s = B.to_mont_limbs([B.fr_random(B.Xoshiro256ss(0x1818))])[0]
    params = ParamsKZG.setup_from_toxic_waste(ctx, k, s)
    _, gl = params.download()
    vecs = [full_range_words(n, 180 + j) for j in range(3)]
    dev = [ctx.to_device(v) for v in vecs]
    res = ctx.msm_batch_dev([d.ptr for d in dev], params.g_lagrange_dev, n)
    for j, v in enumerate(vecs):
        assert np.array_equal(OC.g1_to_affine(res[j]), OC.g1_to_affine(OC.best_multiexp(v, gl))), "MSM %d differs" % j
    params.close()


@pytest.mark.parametrize("n", [300_001, 400_003, 3_200_001])  # 4, 8 and 16 elements per lane
def test_batch_invert_full_range_words(ctx, n):
    """The words are a R mod p for some a, so the result words must be R^2 / w mod r; zeros stay zero."""
    w = full_range_words(n, n & 0xFFFF)
    w[::7] = 0
    got = ctx.batch_invert(w.copy())
    assert got.shape == w.shape and not got[::7].any()
    rs = np.random.RandomState(n)
    blk = max(1, n // 16)
    rows = np.unique(np.concatenate([np.arange(0, 40), np.arange(n - 40, n), rs.randint(0, n, size=1500),
                                     np.arange(n // 4, n // 4 + 200), np.arange(n // 2, n // 2 + 200), [n // 2 + blk - 1]]))
    r2 = pow(2, 512, B.R_MOD)
    for i in rows:
        x = sum(int(w[i, q]) << (64 * q) for q in range(4))
        y = sum(int(got[i, q]) << (64 * q) for q in range(4))
        assert y == (r2 * pow(x, -1, B.R_MOD) % B.R_MOD if x else 0), i

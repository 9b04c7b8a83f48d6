"""The short-MSM kernel's resources, read from the built gfx950 code object (tools/code_object_audit.py): no scratch memory,
and the LDS figure DESIGN.md section 0a records.  (The path adds no host fold: its results have the layout of a plain 8-bit-window
launch and are folded by msm_fold_windows.)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# static LDS of msm_short_kernel: histogram, cursors (128 words each) and the 129 list starts; the digit bytes (one per term,
# 4 112 B for the 4097 terms of [b_0] / [p]) are dynamic LDS on top of it
SHORT_STATIC_LDS = 1552
SHORT_DYNAMIC_LDS_4097 = 4112
NTT_PASS_LDS_PER_CU = 4 * 37 * 1024
LDS_PER_CU = 160 * 1024


def _short_kernel():
    import code_object_audit as audit

    assert os.path.exists(audit.LIB), "build the library first (python -m sha2_on_cq_halo2_amd.build)"
    ks = {name: k for name, k in audit.kernels().items() if "msm_short_kernel" in name}
    assert len(ks) == 1, sorted(ks)
    return next(iter(ks.values()))


def test_short_msm_kernel_does_not_spill():
    k = _short_kernel()
    assert k["scratch"] == 0, k
    assert k["threads"] == 256, k


def test_short_msm_kernel_lds_is_the_documented_figure_and_fits_beside_the_ntt_passes():
    k = _short_kernel()
    assert k["lds"] == SHORT_STATIC_LDS, k
    assert k["lds"] + SHORT_DYNAMIC_LDS_4097 <= LDS_PER_CU - NTT_PASS_LDS_PER_CU

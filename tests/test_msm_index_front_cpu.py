"""The index front's two kernels, read from the built gfx950 code object (tools/code_object_audit.py): no scratch memory, and
the static LDS the source declares -- the tile's hash table, whatever the number of buckets."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

INDEX_SLOTS = 2 * 256 * 8  # msm_sort.hip: two slots per row of a tile
COUNT_LDS = 2 * INDEX_SLOTS * 4 + 4  # keys, counts, the tile's total
PLACE_LDS = 2 * INDEX_SLOTS * 4      # keys, runs


def _kernel(name):
    import code_object_audit as audit

    assert os.path.exists(audit.LIB), "build the library first (python -m sha2_on_cq_halo2_amd.build)"
    ks = {n: k for n, k in audit.kernels().items() if name in n}
    assert len(ks) == 1, sorted(ks)
    return next(iter(ks.values()))


def test_index_front_kernels_do_not_spill():
    for name in ("msm_index_count_kernel", "msm_index_place_kernel"):
        k = _kernel(name)
        assert k["scratch"] == 0, k
        assert k["threads"] == 256, k


def test_index_front_lds_is_what_the_source_declares():
    assert _kernel("msm_index_count_kernel")["lds"] == COUNT_LDS
    assert _kernel("msm_index_place_kernel")["lds"] == PLACE_LDS


def test_index_scalars_kernel_is_gone():
    import code_object_audit as audit

    assert not [n for n in audit.kernels() if "msm_index_scalars" in n]

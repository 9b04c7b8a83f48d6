"""CPU: the four stage entry points (cq_permutation_commit_dev, cq_lookup_commit_product_dev, cq_evaluate_h_dev,
cq_multiopen_dev) are declared in include/cq_halo2.h, exported by the library, and bound in the package's modules with the
argument counts the header states.  The header is parsed the way tests/test_abi_cpu.py does (sha2_on_cq_halo2_amd._lib)."""
import ast
import glob
import os

from sha2_on_cq_halo2_amd import _lib, header_symbols, load

STAGES = {"cq_permutation_commit_dev": 9, "cq_lookup_commit_product_dev": 11, "cq_evaluate_h_dev": 13, "cq_multiopen_dev": 4}
ACCESSORS = ("cq_pk_permutation_sets", "cq_pk_legacy_lookups")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_declares_the_stage_entry_points_and_the_library_exports_them():
    syms = header_symbols()
    protos = {p.name: p for p in _lib.header_prototypes()}
    lib = load()
    for name, argc in STAGES.items():
        assert name in syms, name
        assert protos[name].ret == "int" and len(protos[name].params) == argc, protos[name]
        assert protos[name].params[0] == "cq_pk* pk"
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == argc
    # the transcript callbacks cross the ABI as function-pointer typedefs
    assert {"cq_squeeze_challenge_fn", "cq_write_point_fn"} <= _lib.header_fnptr_typedefs()
    for name in ACCESSORS:  # the counts that size the stage calls' buffers
        assert name in syms and hasattr(lib, name), name


def test_api_binds_every_stage_with_the_headers_argument_count():
    seen = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "sha2_on_cq_halo2_amd", "*.py"))):  # every module of the binding
        for node in ast.walk(ast.parse(open(path).read())):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in STAGES:
                assert not any(isinstance(a, ast.Starred) for a in node.args) and not any(k.arg is None for k in node.keywords), path
                seen.setdefault(node.func.attr, []).append(len(node.args) + len(node.keywords))
    for name, argc in STAGES.items():
        assert seen.get(name) == [argc], (name, seen.get(name))
    from sha2_on_cq_halo2_amd import ProvingKey

    for method in ("permutation_commit", "lookup_commit_product", "evaluate_h", "multiopen"):
        assert callable(getattr(ProvingKey, method)), method

"""Host-side mirror of the reference's operator interface over the C ABI (ctypes): the import surface.

Names, argument meaning and error behaviour follow the Rust functions they stand for
(halo2_proofs/src/arithmetic.rs, poly/domain.rs, poly/kzg/commitment.rs); contract
violations that panic in Rust raise `CqError` here.  The classes live in context.py (`Context`, `DevBuf`),
params.py (`ParamsKZG`, `G2Srs`, `TableConfig`, `StaticTable`, `EvaluationDomain`) and proving_key.py (`ProvingKey`,
the witness checker); _marshal.py holds the array and ctypes helpers and what is derived from include/cq_halo2.h.
"""
from ._lib import CqError, load  # noqa: F401
from ._marshal import (FAIL_GATE, FAIL_GATE_POISONED, FAIL_LOOKUP, FAIL_PERMUTATION, FAIL_STATIC_LOOKUP, FR_MODULUS,  # noqa: F401
                       FR_ROOT_OF_UNITY, FR_S, PROF_G1_DECOMPRESS, PROF_G2_DECOMPRESS, PROF_MSM_ACCUMULATE, PROF_MSM_ENTRIES,
                       PROF_NTT_PASS, RCCL_UNIQUE_ID_BYTES, SERDE_PROCESSED, SERDE_RAW_BYTES, SERDE_RAW_BYTES_UNCHECKED, SHA_CH,
                       SHA_MAJ, SHA_ROT0, SHA_ROT1, _ALLGATHER_T, _BCAST_T, _EXCHANGE_T, _SQUEEZE_T, _WRITE_POINT_T, _BufferRng,
                       _CqAssignedColumn, _CqCircuit, _CqOpenQuery, _CqOpenTranscript, _CqPlonk, _CqXfer, domain_omega,
                       domain_omega_int, fr_from_mont, fr_to_mont)
from .context import Context, DevBuf, rccl_unique_id  # noqa: F401
from .params import EvaluationDomain, G2Srs, ParamsKZG, StaticTable, TableConfig  # noqa: F401
from .proving_key import ProvingKey, WitnessError, WitnessFailure, _lower_plonk  # noqa: F401
from .sha256_circuit import Sha256Circuit  # noqa: F401  (last: its constructor reaches sha_circuit, which imports this module)
from .sha256_segments import (HmacSha256Circuit, Sha224Circuit, Sha256BatchCircuit, Sha256dCircuit, Sha256MerkleCircuit,  # noqa: F401
                              Sha256MerklePathCircuit, Sha256MidstateCircuit, Sha256SegmentsCircuit)
from .sha256_varlen import Sha256VarCircuit  # noqa: F401
from .sha256_stream import Sha256Stream, link  # noqa: F401
from .sha512_circuit import Sha384Circuit, Sha512BatchCircuit, Sha512Circuit  # noqa: F401
# the plans of the wired SHA-512 segments: `batch`, `merkle_tree` and `midstate` are sha512_segments', not sha256_segments'
from .sha512_segments import (Sha512_256Circuit, Sha512dCircuit, Sha512MerkleCircuit, Sha512MidstateCircuit, Sha512SegmentsCircuit,  # noqa: F401
                              batch, double_sha512, merkle_tree, midstate, sha512_256)
from .sha512_xor import HmacSha384Circuit, HmacSha512Circuit, Sha512XorSegmentsCircuit, hmac_sha512  # noqa: F401

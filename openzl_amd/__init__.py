"""openzl_amd -- MI355X (gfx950) MSM / NTT backend for OpenZL's arkworks Groth16 plugin path.

The product is the C-ABI shared library `libzl_backend.so` (include/zl_backend.h).  This package holds its HIP
sources (csrc/), the build driver (build.py) and a thin ctypes binding (backend.py) used by the tests and the
bench; it never falls back to a CPU implementation: without the HIP library or without a GPU it raises.
"""
from .backend import Backend, MultiBackend, BackendError, load_library, CURVES, ZL_BLS12_381, ZL_BN254, ZL_G1, ZL_G2  # noqa: F401
from .backend import ZL_MONT, ZL_COSET, ZL_INVERSE, ZL_CHECK  # noqa: F401
from .backend import Circuit, Groth16Keys, MerkleForest, poseidon_permute, pairing, pairing_product  # noqa: F401
from .backend import (poseidon_permute_batch_host, poseidon_hash2_host, poseidon_chain_host, poseidon_merkle_nodes, poseidon_merkle_root_host,  # noqa: F401
                      poseidon_merkle_build_host, poseidon_merkle_paths_host, poseidon_roots_from_paths_host, poseidon_chain_assignment_elems,
                      poseidon_chain_assignments_host, poseidon_merkle_assignment_elems, poseidon_merkle_assignments_host, poseidon_hash_host, poseidon_spec, poseidon_constants)
from .backend import (poseidon_hash_assignment_elems, poseidon_hash_assignments_host, poseidon_merkle_leaf_assignment_elems,  # noqa: F401
                      poseidon_merkle_leaf_assignments_host)
from .backend import poseidon_duplex_permutations, poseidon_duplex_encrypt_host, poseidon_duplex_decrypt_host  # noqa: F401
from .backend import poseidon_encrypt_assignment_elems, poseidon_encrypt_assignments_host  # noqa: F401
from .backend import ZL_ED_CHECK_SUBGROUP, ed_params, ed_add_host, ed_scalar_mul_host, hybrid_encrypt_host, hybrid_decrypt_host  # noqa: F401
from .backend import ed_order_bits, ed_scalar_mul_assignment_elems, ed_scalar_mul_assignments_host  # noqa: F401
from .backend import hybrid_encrypt_assignment_elems, hybrid_encrypt_assignments_host  # noqa: F401

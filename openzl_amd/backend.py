"""ctypes binding of include/zl_backend.h.  No compute happens in Python and there is no CPU fallback."""
from __future__ import annotations

import collections
import ctypes as C
import os
from typing import Optional, Tuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libzl_backend.so")

ZL_BLS12_381, ZL_BN254 = 1, 2
ZL_G1, ZL_G2 = 1, 2
ZL_MONT, ZL_COSET, ZL_INVERSE, ZL_CHECK, ZL_MONT_IN, ZL_MONT_OUT = 1, 2, 4, 8, 16, 32
ZL_PARTIAL_WORDS = 64
CURVES = {"bls12_381": ZL_BLS12_381, "bn254": ZL_BN254}
FQ_LIMBS = {ZL_BLS12_381: 6, ZL_BN254: 4}

u64p = C.POINTER(C.c_uint64)
u8p = C.POINTER(C.c_uint8)
i32p = C.POINTER(C.c_int32)

# every symbol include/zl_backend.h declares (tests check the library exports all of them)
ABI_SYMBOLS = [
    "zl_ctx_create", "zl_ctx_destroy", "zl_ctx_fork", "zl_ctx_set_stream", "zl_ctx_sync", "zl_ctx_set_msm_window", "zl_ctx_last_hip_error",
    "zl_strerror", "zl_describe", "zl_bases_upload", "zl_bases_generate", "zl_bases_download", "zl_bases_precompute", "zl_bases_free", "zl_msm",
    "zl_msm_dev", "zl_msm_partial_dev", "zl_msm_batch_partial_dev", "zl_partials_sum", "zl_partial_from_affine", "zl_ntt", "zl_ntt_dev", "zl_ntt_batch_dev", "zl_ntt_cross_dev", "zl_ctx_enable_timing", "zl_last_timing", "zl_groth16_prove", "zl_groth16_last_h", "zl_r1cs_upload", "zl_r1cs_free", "zl_groth16_prove_resident", "zl_groth16_prove_sharded", "zl_circuit_poseidon_chain", "zl_circuit_poseidon_chain_witness", "zl_circuit_free", "zl_circuit_export",
    "zl_circuit_is_satisfied", "zl_poseidon_permute", "zl_groth16_compile", "zl_groth16_keys_free", "zl_groth16_keys_pk",
    "zl_groth16_keys_trapdoor", "zl_groth16_prove_circuit", "zl_groth16_prove_circuits", "zl_ctx_drop_lanes", "zl_groth16_verify", "zl_pairing",
    "zl_ctx_create_multi", "zl_mctx_destroy", "zl_mctx_size", "zl_mctx_ctx", "zl_mctx_uses_rccl", "zl_mctx_last_rccl_error", "zl_msm_sharded", "zl_ntt_sharded",
    "zl_point_bytes", "zl_point_to_bytes", "zl_point_from_bytes", "zl_groth16_proof_bytes", "zl_groth16_proof_to_bytes", "zl_groth16_proof_from_bytes",
    "zl_point_bytes_uncompressed", "zl_point_to_bytes_uncompressed", "zl_point_from_bytes_uncompressed", "zl_groth16_keys_to_bytes", "zl_groth16_keys_from_bytes", "zl_groth16_keys_parse",
    "zl_groth16_vk_to_bytes", "zl_pairing_product", "zl_groth16_verify_batch",
    "zl_points_from_bytes_batch", "zl_groth16_proofs_from_bytes_batch", "zl_groth16_verify_batch_bytes", "zl_msm_multi_dev", "zl_groth16_prove_batch",
    "zl_pairing_products",
    "zl_poseidon_permute_batch", "zl_poseidon_hash2_batch", "zl_poseidon_hash2_batch_dev", "zl_poseidon_chain_batch", "zl_poseidon_merkle_nodes",
    "zl_poseidon_merkle_build_dev", "zl_poseidon_merkle_build", "zl_poseidon_merkle_root", "zl_poseidon_merkle_paths_dev", "zl_poseidon_merkle_paths",
    "zl_poseidon_merkle_roots_from_paths",
    "zl_poseidon_chain_assignment_elems", "zl_poseidon_chain_assignments_dev", "zl_poseidon_chain_assignments", "zl_groth16_prove_batch_dev",
    "zl_groth16_prove_poseidon_chains",
    "zl_circuit_poseidon_merkle", "zl_circuit_poseidon_merkle_witness", "zl_poseidon_merkle_assignment_elems", "zl_poseidon_merkle_assignments",
    "zl_poseidon_merkle_assignments_dev", "zl_poseidon_merkle_member_assignments_dev", "zl_groth16_prove_merkle_paths", "zl_groth16_prove_merkle_members",
    "zl_poseidon_spec", "zl_poseidon_permute_w", "zl_poseidon_constants", "zl_poseidon_permute_batch_w", "zl_poseidon_hash_batch", "zl_poseidon_hash_batch_dev",
    "zl_merkle_forest_create", "zl_merkle_forest_destroy", "zl_merkle_forest_describe", "zl_merkle_forest_lens", "zl_merkle_forest_append",
    "zl_merkle_forest_append_dev", "zl_merkle_forest_roots", "zl_merkle_forest_paths", "zl_merkle_forest_tree_nodes", "zl_merkle_forest_download",
    "zl_merkle_forest_member_assignments_dev", "zl_groth16_prove_forest_members",
    "zl_circuit_poseidon_hash", "zl_circuit_poseidon_hash_witness", "zl_circuit_poseidon_merkle_leaf", "zl_circuit_poseidon_merkle_leaf_witness",
    "zl_poseidon_hash_assignment_elems", "zl_poseidon_merkle_leaf_assignment_elems", "zl_poseidon_hash_assignments", "zl_poseidon_hash_assignments_dev",
    "zl_poseidon_merkle_leaf_assignments", "zl_poseidon_merkle_leaf_assignments_dev", "zl_poseidon_merkle_leaf_member_assignments_dev",
    "zl_groth16_prove_poseidon_hashes", "zl_groth16_prove_merkle_leaf_paths", "zl_groth16_prove_merkle_leaf_members",
    "zl_poseidon_duplex_permutations", "zl_poseidon_duplex_encrypt_batch", "zl_poseidon_duplex_decrypt_batch", "zl_poseidon_duplex_encrypt_batch_dev",
    "zl_poseidon_duplex_decrypt_batch_dev", "zl_circuit_poseidon_encrypt", "zl_circuit_poseidon_encrypt_witness",
    "zl_poseidon_encrypt_assignment_elems", "zl_poseidon_encrypt_assignments", "zl_poseidon_encrypt_assignments_dev", "zl_groth16_prove_poseidon_encryptions",
    "zl_ed_params", "zl_ed_add", "zl_ed_scalar_mul", "zl_ed_scalar_mul_batch", "zl_ed_scalar_mul_batch_dev",
    "zl_hybrid_encrypt_batch", "zl_hybrid_encrypt_batch_dev", "zl_hybrid_decrypt_batch", "zl_hybrid_decrypt_batch_dev",
    "zl_circuit_ed_scalar_mul", "zl_circuit_ed_scalar_mul_witness", "zl_circuit_witness_only_compatible", "zl_ed_scalar_mul_assignment_elems",
    "zl_ed_scalar_mul_assignments", "zl_ed_scalar_mul_assignments_dev", "zl_groth16_prove_ed_scalar_muls",
    "zl_circuit_hybrid_encrypt", "zl_circuit_hybrid_encrypt_witness", "zl_hybrid_encrypt_assignment_elems", "zl_hybrid_encrypt_assignments",
    "zl_hybrid_encrypt_assignments_dev", "zl_groth16_prove_hybrid_encryptions",
]
ZL_ED_CHECK_SUBGROUP = 1


class BackendError(RuntimeError):
    def __init__(self, code: int, what: str, msg: str = ""):
        super().__init__(f"{what} failed: {code} ({msg})")
        self.code = code


class Timing(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("dominant_ms", C.c_float), ("launches", C.c_uint32), ("window_bits", C.c_uint32),
                ("entries", C.c_uint64)]


class R1csC(C.Structure):
    _fields_ = [("n_constraints", C.c_uint32), ("n_instance", C.c_uint32), ("n_witness", C.c_uint32),
                ("row_ptr", C.POINTER(C.c_uint32) * 3), ("col", C.POINTER(C.c_uint32) * 3), ("val", u64p * 3)]


class G16PkC(C.Structure):
    _fields_ = [("curve", C.c_int), ("a_query", C.c_uint64), ("b_g1_query", C.c_uint64), ("h_query", C.c_uint64), ("l_query", C.c_uint64),
                ("b_g2_query", C.c_uint64), ("alpha_g1", u64p), ("beta_g1", u64p), ("delta_g1", u64p), ("beta_g2", u64p), ("delta_g2", u64p)]


class G16ShardC(C.Structure):
    _fields_ = [("a_query", C.c_uint64), ("b_g1_query", C.c_uint64), ("h_query", C.c_uint64), ("l_query", C.c_uint64), ("b_g2_query", C.c_uint64),
                ("var_first", C.c_size_t), ("var_count", C.c_size_t), ("wit_first", C.c_size_t), ("wit_count", C.c_size_t), ("h_first", C.c_size_t),
                ("h_count", C.c_size_t)]


class G16ProofC(C.Structure):
    _fields_ = [("a", C.c_uint64 * 12), ("b", C.c_uint64 * 24), ("c", C.c_uint64 * 12), ("a_inf", C.c_uint8), ("b_inf", C.c_uint8),
                ("c_inf", C.c_uint8)]


_lib = None


def load_library(path: Optional[str] = None):
    """Load libzl_backend.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("ZL_BACKEND_LIB") or LIB_PATH  # ZL_BACKEND_LIB: developer A/B of two builds in one gpurun call
    if not os.path.exists(p):
        raise FileNotFoundError(f"{p} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(p)
    vp = C.c_void_p
    L.zl_ctx_create.argtypes = [C.POINTER(vp), C.c_int]
    L.zl_ctx_destroy.argtypes = [vp]
    L.zl_ctx_fork.argtypes = [vp, C.POINTER(vp)]
    L.zl_ctx_destroy.restype = None
    L.zl_ctx_set_stream.argtypes = [vp, vp]
    L.zl_ctx_sync.argtypes = [vp]
    L.zl_ctx_set_msm_window.argtypes = [vp, C.c_int]
    L.zl_ctx_last_hip_error.argtypes = [vp]
    L.zl_strerror.argtypes = [C.c_int]
    L.zl_strerror.restype = C.c_char_p
    L.zl_describe.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.zl_bases_upload.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t, C.c_size_t, C.c_long, C.c_uint, u64p]
    L.zl_bases_generate.argtypes = [vp, C.c_int, C.c_int, u64p, C.c_size_t, u64p]
    L.zl_bases_download.argtypes = [vp, C.c_uint64, C.c_size_t, C.c_size_t, u64p]
    L.zl_bases_free.argtypes = [vp, C.c_uint64]
    L.zl_bases_precompute.argtypes = [vp, C.c_uint64, C.c_int]
    L.zl_msm.argtypes = [vp, C.c_uint64, C.c_size_t, u64p, C.c_size_t, u64p, u8p]
    L.zl_msm_dev.argtypes = [vp, C.c_uint64, C.c_size_t, vp, C.c_size_t, u64p, u8p]
    L.zl_msm_partial_dev.argtypes = [vp, C.c_uint64, C.c_size_t, vp, C.c_size_t, u64p]
    L.zl_partials_sum.argtypes = [C.c_int, C.c_int, u64p, C.c_size_t, u64p, u8p]
    L.zl_partial_from_affine.argtypes = [C.c_int, C.c_int, u64p, u64p]
    L.zl_msm_batch_partial_dev.argtypes = [vp, C.c_uint64, C.c_size_t, C.POINTER(C.c_void_p), C.c_size_t, C.c_size_t, u64p]
    L.zl_msm_multi_dev.argtypes = [vp, C.c_uint64, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_size_t, u64p, u8p]
    L.zl_ntt.argtypes = [vp, C.c_int, u64p, C.c_uint, C.c_uint]
    L.zl_ntt_dev.argtypes = [vp, C.c_int, vp, C.c_uint, C.c_uint]
    L.zl_ntt_cross_dev.argtypes = [vp, C.c_int, vp, C.c_uint, C.c_uint, C.c_uint, C.c_uint]
    L.zl_ntt_batch_dev.argtypes = [vp, C.c_int, vp, C.c_uint, C.c_uint, C.c_uint, C.c_size_t]
    L.zl_ctx_enable_timing.argtypes = [vp, C.c_int]
    L.zl_last_timing.argtypes = [vp, C.POINTER(Timing)]
    L.zl_groth16_prove.argtypes = [vp, C.POINTER(G16PkC), C.POINTER(R1csC), u64p, u64p, u64p, C.POINTER(G16ProofC)]
    L.zl_groth16_prove_sharded.argtypes = [vp, C.POINTER(G16PkC), C.POINTER(G16ShardC), C.c_uint64, u64p, C.c_uint, u64p, u64p, C.POINTER(G16ProofC)]
    L.zl_groth16_last_h.argtypes = [vp, u64p, C.c_size_t]
    L.zl_r1cs_upload.argtypes = [vp, C.c_int, C.POINTER(R1csC), C.POINTER(C.c_uint64)]
    L.zl_r1cs_free.argtypes = [vp, C.c_uint64]
    L.zl_groth16_prove_resident.argtypes = [vp, C.POINTER(G16PkC), C.c_uint64, u64p, C.c_uint, u64p, u64p, C.POINTER(G16ProofC)]
    L.zl_groth16_prove_batch.argtypes = [vp, C.POINTER(G16PkC), C.c_uint64, u64p, C.c_uint, u64p, u64p, C.c_size_t, C.POINTER(G16ProofC)]
    L.zl_groth16_prove_batch_dev.argtypes = [vp, C.POINTER(G16PkC), C.c_uint64, vp, C.c_uint, u64p, u64p, C.c_size_t, C.POINTER(G16ProofC)]
    L.zl_groth16_prove_poseidon_chains.argtypes = [vp, C.POINTER(G16PkC), C.c_uint64, C.c_uint32, u64p, u64p, u64p, u64p, C.c_size_t, C.POINTER(G16ProofC), u64p]
    L.zl_circuit_poseidon_chain.argtypes = [C.c_int, C.c_uint32, u64p, u64p, C.POINTER(vp)]
    L.zl_circuit_free.argtypes = [vp]
    L.zl_circuit_free.restype = None
    L.zl_circuit_export.argtypes = [vp, C.POINTER(R1csC), C.POINTER(u64p)]
    L.zl_circuit_poseidon_chain_witness.argtypes = L.zl_circuit_poseidon_chain.argtypes
    L.zl_circuit_is_satisfied.argtypes = [vp]
    L.zl_poseidon_permute.argtypes = [C.c_int, u64p]
    L.zl_poseidon_permute_batch.argtypes = [vp, C.c_int, u64p, C.c_size_t]
    L.zl_poseidon_hash2_batch.argtypes = [vp, C.c_int, u64p, C.c_size_t, u64p]
    L.zl_poseidon_hash2_batch_dev.argtypes = [vp, C.c_int, vp, C.c_size_t, vp]
    L.zl_poseidon_spec.argtypes = [C.c_uint, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_uint), u64p]
    L.zl_poseidon_permute_w.argtypes = [C.c_int, C.c_uint, u64p]
    L.zl_poseidon_constants.argtypes = [C.c_int, C.c_uint, u64p, u64p]
    L.zl_poseidon_permute_batch_w.argtypes = [vp, C.c_int, C.c_uint, u64p, C.c_size_t]
    L.zl_poseidon_hash_batch.argtypes = [vp, C.c_int, C.c_uint, u64p, C.c_size_t, u64p]
    L.zl_poseidon_hash_batch_dev.argtypes = [vp, C.c_int, C.c_uint, vp, C.c_size_t, vp]
    L.zl_poseidon_duplex_permutations.argtypes = [C.c_uint, C.c_size_t, C.c_size_t, C.c_size_t]
    L.zl_poseidon_duplex_permutations.restype = C.c_size_t
    L.zl_poseidon_duplex_encrypt_batch.argtypes = [vp, C.c_int, C.c_uint, u64p, u64p, C.c_size_t, u64p, C.c_size_t, u64p, C.c_size_t, C.c_size_t, u64p, u64p]
    L.zl_poseidon_duplex_decrypt_batch.argtypes = [vp, C.c_int, C.c_uint, u64p, u64p, C.c_size_t, u64p, C.c_size_t, u64p, u64p, C.c_size_t, C.c_size_t, u64p, u8p]
    L.zl_poseidon_duplex_encrypt_batch_dev.argtypes = [vp, C.c_int, C.c_uint, u64p, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, vp, vp]
    L.zl_poseidon_duplex_decrypt_batch_dev.argtypes = [vp, C.c_int, C.c_uint, u64p, vp, C.c_size_t, vp, C.c_size_t, vp, vp, C.c_size_t, C.c_size_t, vp, u8p]
    L.zl_ed_params.argtypes = [C.c_int, u64p, u64p, u64p, u64p]
    L.zl_ed_add.argtypes = [C.c_int, u64p, u64p, u64p]
    L.zl_ed_scalar_mul.argtypes = [C.c_int, u64p, u64p, u64p]
    L.zl_ed_scalar_mul_batch.argtypes = [vp, C.c_int, u64p, C.c_size_t, u64p, C.c_size_t, C.c_size_t, C.c_uint, u64p, u8p]
    L.zl_ed_scalar_mul_batch_dev.argtypes = [vp, C.c_int, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_uint, vp, vp]
    L.zl_hybrid_encrypt_batch.argtypes = [vp, C.c_int, C.c_uint, u64p, u64p, u64p, u64p, C.c_size_t, u64p, C.c_size_t, u64p, C.c_size_t, C.c_size_t, C.c_uint, u64p, u64p,
                                          u64p, u8p]
    L.zl_hybrid_encrypt_batch_dev.argtypes = [vp, C.c_int, C.c_uint, u64p, u64p, vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_uint, vp, vp, vp, vp]
    L.zl_hybrid_decrypt_batch.argtypes = [vp, C.c_int, C.c_uint, u64p, u64p, C.c_size_t, u64p, u64p, C.c_size_t, u64p, u64p, C.c_size_t, C.c_size_t, C.c_uint, u64p, u8p,
                                          u8p]
    L.zl_hybrid_decrypt_batch_dev.argtypes = [vp, C.c_int, C.c_uint, u64p, vp, C.c_size_t, vp, vp, C.c_size_t, vp, vp, C.c_size_t, C.c_size_t, C.c_uint, vp, u8p, vp]
    L.zl_circuit_ed_scalar_mul.argtypes = [C.c_int, C.c_uint, u64p, u64p, C.POINTER(vp)]
    L.zl_circuit_ed_scalar_mul_witness.argtypes = L.zl_circuit_ed_scalar_mul.argtypes
    L.zl_circuit_witness_only_compatible.argtypes = [vp]
    L.zl_ed_scalar_mul_assignment_elems.argtypes = [C.c_int, C.c_uint]
    L.zl_ed_scalar_mul_assignment_elems.restype = C.c_size_t
    L.zl_ed_scalar_mul_assignments.argtypes = [vp, C.c_int, C.c_uint, u64p, C.c_size_t, u64p, C.c_size_t, u64p]
    L.zl_ed_scalar_mul_assignments_dev.argtypes = [vp, C.c_int, C.c_uint, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t]
    L.zl_groth16_prove_ed_scalar_muls.argtypes = [vp, C.POINTER(G16PkC), C.c_uint64, C.c_uint, u64p, C.c_size_t, u64p, u64p, u64p, C.c_size_t, C.POINTER(G16ProofC), u64p]
    L.zl_circuit_hybrid_encrypt.argtypes = [C.c_int, C.c_uint, C.c_uint, u64p, u64p, u64p, u64p, u64p, C.c_size_t, u64p, C.c_size_t, C.POINTER(vp)]
    L.zl_circuit_hybrid_encrypt_witness.argtypes = L.zl_circuit_hybrid_encrypt.argtypes
    L.zl_hybrid_encrypt_assignment_elems.argtypes = [C.c_int, C.c_uint, C.c_uint, C.c_size_t, C.c_size_t]
    L.zl_hybrid_encrypt_assignment_elems.restype = C.c_size_t
    L.zl_hybrid_encrypt_assignments.argtypes = [vp, C.c_int, C.c_uint, C.c_uint, u64p, u64p, u64p, u64p, C.c_size_t, u64p, C.c_size_t, u64p, C.c_size_t, C.c_size_t, u64p]
    L.zl_hybrid_encrypt_assignments_dev.argtypes = [vp, C.c_int, C.c_uint, C.c_uint, u64p, u64p, vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t]
    L.zl_groth16_prove_hybrid_encryptions.argtypes = [vp, C.POINTER(G16PkC), C.c_uint64, C.c_uint, C.c_uint, u64p, u64p, u64p, u64p, C.c_size_t, u64p, C.c_size_t, u64p,
                                                      C.c_size_t, u64p, u64p, C.c_size_t, C.POINTER(G16ProofC), u64p, u64p, u64p]
    L.zl_circuit_poseidon_encrypt.argtypes = [C.c_int, C.c_uint, u64p, u64p, C.c_size_t, u64p, C.c_size_t, u64p, C.c_size_t, C.POINTER(vp)]
    L.zl_circuit_poseidon_encrypt_witness.argtypes = L.zl_circuit_poseidon_encrypt.argtypes
    L.zl_poseidon_encrypt_assignment_elems.argtypes = [C.c_uint, C.c_size_t, C.c_size_t, C.c_size_t]
    L.zl_poseidon_encrypt_assignment_elems.restype = C.c_size_t
    L.zl_poseidon_encrypt_assignments.argtypes = [vp, C.c_int, C.c_uint, u64p, u64p, C.c_size_t, u64p, C.c_size_t, u64p, C.c_size_t, C.c_size_t, u64p]
    L.zl_poseidon_encrypt_assignments_dev.argtypes = [vp, C.c_int, C.c_uint, u64p, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t]
    L.zl_groth16_prove_poseidon_encryptions.argtypes = [vp, C.POINTER(G16PkC), C.c_uint64, C.c_uint, u64p, u64p, C.c_size_t, u64p, C.c_size_t, u64p, C.c_size_t, u64p, u64p,
                                                        C.c_size_t, C.POINTER(G16ProofC), u64p, u64p]
    L.zl_poseidon_chain_batch.argtypes = [vp, C.c_int, u64p, u64p, C.c_uint32, C.c_size_t, u64p]
    L.zl_poseidon_chain_assignment_elems.argtypes = [C.c_uint32]
    L.zl_poseidon_chain_assignment_elems.restype = C.c_size_t
    L.zl_poseidon_chain_assignments_dev.argtypes = [vp, C.c_int, vp, vp, C.c_uint32, C.c_size_t, vp, C.c_size_t]
    L.zl_poseidon_chain_assignments.argtypes = [vp, C.c_int, u64p, u64p, C.c_uint32, C.c_size_t, u64p]
    L.zl_poseidon_merkle_nodes.argtypes = [C.c_size_t, C.c_uint]
    L.zl_poseidon_merkle_nodes.restype = C.c_size_t
    L.zl_poseidon_merkle_build_dev.argtypes = [vp, C.c_int, vp, C.c_size_t, C.c_uint, vp, u64p]
    L.zl_poseidon_merkle_build.argtypes = [vp, C.c_int, u64p, C.c_size_t, C.c_uint, u64p, u64p]
    L.zl_poseidon_merkle_root.argtypes = [vp, C.c_int, u64p, C.c_size_t, C.c_uint, u64p]
    L.zl_poseidon_merkle_paths_dev.argtypes = [vp, C.c_int, vp, C.c_size_t, C.c_uint, u64p, C.c_size_t, u64p]
    L.zl_poseidon_merkle_paths.argtypes = [u64p, C.c_size_t, C.c_uint, u64p, C.c_size_t, u64p]
    L.zl_poseidon_merkle_roots_from_paths.argtypes = [vp, C.c_int, u64p, u64p, u64p, C.c_uint, C.c_size_t, u64p]
    L.zl_circuit_poseidon_merkle.argtypes = [C.c_int, C.c_uint, u64p, C.c_uint64, u64p, C.POINTER(vp)]
    L.zl_circuit_poseidon_merkle_witness.argtypes = L.zl_circuit_poseidon_merkle.argtypes
    L.zl_poseidon_merkle_assignment_elems.argtypes = [C.c_uint]
    L.zl_poseidon_merkle_assignment_elems.restype = C.c_size_t
    L.zl_poseidon_merkle_assignments.argtypes = [vp, C.c_int, u64p, u64p, u64p, C.c_uint, C.c_size_t, u64p]
    L.zl_poseidon_merkle_assignments_dev.argtypes = [vp, C.c_int, vp, u64p, vp, C.c_uint, C.c_size_t, vp, C.c_size_t]
    L.zl_poseidon_merkle_member_assignments_dev.argtypes = [vp, C.c_int, vp, C.c_size_t, C.c_uint, u64p, C.c_size_t, vp, C.c_size_t]
    L.zl_groth16_prove_merkle_paths.argtypes = [vp, C.POINTER(G16PkC), C.c_uint64, C.c_uint, u64p, u64p, u64p, u64p, u64p, C.c_size_t, C.POINTER(G16ProofC), u64p]
    L.zl_groth16_prove_merkle_members.argtypes = [vp, C.POINTER(G16PkC), C.c_uint64, vp, C.c_size_t, C.c_uint, u64p, u64p, u64p, C.c_size_t, C.POINTER(G16ProofC), u64p]
    u32p = C.POINTER(C.c_uint32)
    L.zl_circuit_poseidon_hash.argtypes = [C.c_int, C.c_uint, u64p, C.POINTER(vp)]
    L.zl_circuit_poseidon_hash_witness.argtypes = L.zl_circuit_poseidon_hash.argtypes
    L.zl_circuit_poseidon_merkle_leaf.argtypes = [C.c_int, C.c_uint, C.c_uint, u64p, C.c_uint64, u64p, C.POINTER(vp)]
    L.zl_circuit_poseidon_merkle_leaf_witness.argtypes = L.zl_circuit_poseidon_merkle_leaf.argtypes
    L.zl_poseidon_hash_assignment_elems.argtypes = [C.c_uint]
    L.zl_poseidon_hash_assignment_elems.restype = C.c_size_t
    L.zl_poseidon_merkle_leaf_assignment_elems.argtypes = [C.c_uint, C.c_uint]
    L.zl_poseidon_merkle_leaf_assignment_elems.restype = C.c_size_t
    L.zl_poseidon_hash_assignments.argtypes = [vp, C.c_int, C.c_uint, u64p, C.c_size_t, u64p]
    L.zl_poseidon_hash_assignments_dev.argtypes = [vp, C.c_int, C.c_uint, vp, C.c_size_t, vp, C.c_size_t]
    L.zl_poseidon_merkle_leaf_assignments.argtypes = [vp, C.c_int, C.c_uint, u64p, u64p, u64p, C.c_uint, C.c_size_t, u64p]
    L.zl_poseidon_merkle_leaf_assignments_dev.argtypes = [vp, C.c_int, C.c_uint, vp, u64p, vp, C.c_uint, C.c_size_t, vp, C.c_size_t]
    L.zl_poseidon_merkle_leaf_member_assignments_dev.argtypes = [vp, C.c_int, C.c_uint, vp, vp, C.c_size_t, C.c_uint, u64p, C.c_size_t, vp, C.c_size_t]
    L.zl_groth16_prove_poseidon_hashes.argtypes = [vp, C.POINTER(G16PkC), C.c_uint64, C.c_uint, u64p, u64p, u64p, C.c_size_t, C.POINTER(G16ProofC), u64p]
    L.zl_groth16_prove_merkle_leaf_paths.argtypes = [vp, C.POINTER(G16PkC), C.c_uint64, C.c_uint, C.c_uint, u64p, u64p, u64p, u64p, u64p, C.c_size_t,
                                                     C.POINTER(G16ProofC), u64p]
    L.zl_groth16_prove_merkle_leaf_members.argtypes = [vp, C.POINTER(G16PkC), C.c_uint64, C.c_uint, vp, vp, C.c_size_t, C.c_uint, u64p, u64p, u64p, C.c_size_t,
                                                       C.POINTER(G16ProofC), u64p]
    L.zl_merkle_forest_create.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint, C.c_size_t, C.POINTER(vp)]
    L.zl_merkle_forest_destroy.argtypes = [vp]
    L.zl_merkle_forest_destroy.restype = None
    L.zl_merkle_forest_describe.argtypes = [vp, u32p, C.POINTER(C.c_uint), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.zl_merkle_forest_lens.argtypes = [vp, u64p]
    L.zl_merkle_forest_append.argtypes = [vp, u32p, u64p, C.c_size_t]
    L.zl_merkle_forest_append_dev.argtypes = [vp, u32p, vp, C.c_size_t]
    L.zl_merkle_forest_roots.argtypes = [vp, u64p]
    L.zl_merkle_forest_paths.argtypes = [vp, u32p, u64p, C.c_size_t, u64p]
    L.zl_merkle_forest_tree_nodes.argtypes = [vp, C.c_uint32, C.POINTER(vp)]
    L.zl_merkle_forest_download.argtypes = [vp, C.c_uint32, u64p]
    L.zl_merkle_forest_member_assignments_dev.argtypes = [vp, u32p, u64p, C.c_size_t, vp, C.c_size_t]
    L.zl_groth16_prove_forest_members.argtypes = [vp, C.POINTER(G16PkC), C.c_uint64, vp, u32p, u64p, u64p, u64p, C.c_size_t, C.POINTER(G16ProofC), u64p]
    L.zl_groth16_compile.argtypes = [vp, vp, C.c_uint64, C.POINTER(vp)]
    L.zl_groth16_keys_free.argtypes = [vp]
    L.zl_groth16_keys_free.restype = None
    L.zl_groth16_keys_pk.argtypes = [vp, C.POINTER(G16PkC)]
    L.zl_groth16_keys_trapdoor.argtypes = [vp, u64p]
    L.zl_groth16_prove_circuit.argtypes = [vp, vp, vp, C.c_uint64, C.POINTER(G16ProofC), u64p, u64p]
    L.zl_groth16_prove_circuits.argtypes = [vp, vp, C.POINTER(vp), u64p, C.c_size_t, C.POINTER(G16ProofC)]
    L.zl_ctx_drop_lanes.argtypes = [vp]
    L.zl_groth16_verify.argtypes = [vp, u64p, C.c_size_t, C.POINTER(G16ProofC), C.POINTER(C.c_int)]
    L.zl_pairing.argtypes = [C.c_int, u64p, u64p, u64p]
    L.zl_pairing_product.argtypes = [vp, C.c_int, u64p, u64p, C.c_size_t, u64p]
    L.zl_pairing_products.argtypes = [vp, C.c_int, u64p, u64p, C.c_size_t, C.c_size_t, u64p, i32p]
    L.zl_groth16_verify_batch.argtypes = [vp, vp, u64p, C.c_size_t, C.POINTER(G16ProofC), C.c_size_t, u64p, C.POINTER(C.c_int), u8p]
    L.zl_points_from_bytes_batch.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t, u64p, u8p, i32p]
    L.zl_groth16_proofs_from_bytes_batch.argtypes = [vp, C.c_int, vp, C.c_size_t, C.POINTER(G16ProofC), i32p]
    L.zl_groth16_verify_batch_bytes.argtypes = [vp, vp, u64p, C.c_size_t, vp, C.c_size_t, u64p, C.POINTER(C.c_int), u8p, i32p]
    L.zl_point_bytes.argtypes = [C.c_int, C.c_int]
    L.zl_point_bytes.restype = C.c_size_t
    L.zl_point_to_bytes.argtypes = [C.c_int, C.c_int, u64p, C.c_uint8, u8p]
    L.zl_point_from_bytes.argtypes = [C.c_int, C.c_int, u8p, u64p, u8p]
    L.zl_groth16_proof_bytes.argtypes = [C.c_int]
    L.zl_groth16_proof_bytes.restype = C.c_size_t
    L.zl_groth16_proof_to_bytes.argtypes = [C.c_int, C.POINTER(G16ProofC), u8p]
    L.zl_groth16_proof_from_bytes.argtypes = [C.c_int, u8p, C.c_size_t, C.POINTER(G16ProofC)]
    L.zl_point_bytes_uncompressed.argtypes = [C.c_int, C.c_int]
    L.zl_point_bytes_uncompressed.restype = C.c_size_t
    L.zl_point_to_bytes_uncompressed.argtypes = [C.c_int, C.c_int, u64p, C.c_uint8, u8p]
    L.zl_point_from_bytes_uncompressed.argtypes = [C.c_int, C.c_int, u8p, C.c_int, u64p, u8p]
    L.zl_groth16_keys_to_bytes.argtypes = [vp, u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.zl_groth16_keys_from_bytes.argtypes = [vp, C.c_int, u8p, C.c_size_t, C.c_uint, C.POINTER(vp)]
    L.zl_groth16_keys_parse.argtypes = [C.c_int, u8p, C.c_size_t, C.c_uint]
    L.zl_groth16_vk_to_bytes.argtypes = [vp, u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    # multi-GPU in one process
    L.zl_ctx_create_multi.argtypes = [C.POINTER(vp), C.POINTER(C.c_int), C.c_int]
    L.zl_mctx_destroy.argtypes = [vp]
    L.zl_mctx_destroy.restype = None
    L.zl_mctx_size.argtypes = [vp]
    L.zl_mctx_ctx.argtypes = [vp, C.c_int]
    L.zl_mctx_ctx.restype = vp
    L.zl_mctx_uses_rccl.argtypes = [vp]
    L.zl_mctx_last_rccl_error.argtypes = [vp]
    L.zl_msm_sharded.argtypes = [vp, u64p, C.POINTER(C.c_size_t), C.POINTER(vp), C.POINTER(C.c_size_t), u64p, u8p]
    L.zl_ntt_sharded.argtypes = [vp, C.c_int, C.POINTER(vp), C.c_uint, C.c_uint]
    # test-only hooks (include/zl_backend_test.h)
    u32p = C.POINTER(C.c_uint32)
    L.zl_test_poseidon_permute_dev.argtypes = [vp, C.c_int, u64p]
    L.zl_test_fp28_op.argtypes = [vp, C.c_int, u32p, C.c_size_t, u32p]
    L.zl_test_fp28_bn_op.argtypes = [vp, C.c_int, u32p, C.c_size_t, u32p]
    L.zl_test_fp_op.argtypes = [vp, C.c_int, C.c_int, C.c_int, u32p, C.c_size_t, u32p]
    L.zl_test_pairing_product.argtypes = [C.c_int, C.c_size_t, u64p, u64p, u64p]
    L.zl_test_miller_dev.argtypes = [vp, C.c_int, C.c_size_t, u64p, u64p, u64p]
    L.zl_test_pairing_product_scaled.argtypes = [vp, C.c_int, C.c_size_t, u64p, u64p, u64p, u64p]
    L.zl_test_final_exp.argtypes = [C.c_int, u64p, u64p]
    L.zl_test_final_exp_dev.argtypes = [vp, C.c_int, C.c_size_t, u64p, u64p, u8p]
    L.zl_test_fq12_inverse.argtypes = [C.c_int, u64p, u64p, u8p]
    L.zl_test_fq12_zeta.argtypes = [C.c_int, u64p]
    L.zl_test_verify_batch_host.argtypes = [C.c_int, u64p, u64p, u64p, u64p, u64p, C.c_size_t, C.POINTER(G16ProofC), u64p, C.c_size_t, u64p,
                                            C.POINTER(C.c_int), u8p]
    L.zl_test_point_op.argtypes = [vp, C.c_int, C.c_int, C.c_int, u32p, C.c_size_t, u32p]
    L.zl_test_fp2pair_op.argtypes = [vp, C.c_int, C.c_int, u32p, C.c_size_t, u32p]
    L.zl_test_point_form_op.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, u32p, C.c_size_t, u32p]
    L.zl_test_circuit_tweak.argtypes = [vp]
    L.zl_test_fq_mul_rate.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.zl_test_fr28_op.argtypes = [vp, C.c_int, C.c_int, C.c_int, u32p, C.c_size_t, u32p]
    L.zl_test_fr29_op.argtypes = [vp, C.c_int, C.c_int, C.c_int, u32p, C.c_size_t, u32p]
    L.zl_test_poseidon_permute_dev28r.argtypes = [vp, C.c_int, u64p]
    L.zl_test_fq_mul_clock.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.zl_test_acc_clock.argtypes = [vp, C.c_int]
    L.zl_test_acc_clock_read.argtypes = [vp, C.POINTER(C.c_double)]
    L.zl_test_clock_probe_launch.argtypes = [vp, C.c_uint]
    L.zl_test_clock_probe_read.argtypes = [vp, C.POINTER(C.c_double)]
    L.zl_test_ntt_plan.argtypes = [C.c_uint, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    L.zl_test_ntt_fit_beside.argtypes = [vp, C.c_int]
    L.zl_test_decode_points_host.argtypes = [C.c_int, C.c_int, vp, C.c_size_t, u64p, u8p, i32p]
    L.zl_test_fq2_sqrt.argtypes = [vp, C.c_int, u64p, C.c_size_t, u64p, u8p]
    # (zl_test_endo_split / _inf: hook_endo_split declares them where it calls them)
    if path is None:
        _lib = L
    return L


def _p64(a: np.ndarray):
    assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"], "need contiguous uint64"
    return a.ctypes.data_as(u64p)


def _r1cs_struct(r1cs: dict):
    """R1csC over r1cs's arrays + the contiguous copies it points into (keep them alive for the call)"""
    cs = R1csC()
    cs.n_constraints, cs.n_instance, cs.n_witness = r1cs["n_constraints"], r1cs["n_instance"], r1cs["n_witness"]
    keep = []
    for m, key in enumerate("ABC"):
        ptr, col, val = (np.ascontiguousarray(x, dtype=t) for x, t in zip(r1cs[key], (np.uint32, np.uint32, np.uint64)))
        keep += [ptr, col, val]
        cs.row_ptr[m] = ptr.ctypes.data_as(C.POINTER(C.c_uint32))
        cs.col[m] = col.ctypes.data_as(C.POINTER(C.c_uint32))
        cs.val[m] = val.ctypes.data_as(u64p)
    return cs, keep


def _pk_struct(curve: int, pk: dict):
    pkc = G16PkC()
    pkc.curve = curve
    keep = []
    for k in ("a_query", "b_g1_query", "h_query", "l_query", "b_g2_query"):
        setattr(pkc, k, pk[k])
    for k in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2"):
        arr = np.ascontiguousarray(pk[k], dtype=np.uint64)
        keep.append(arr)
        setattr(pkc, k, arr.ctypes.data_as(u64p))
    return pkc, keep


def _bytes_view(data, offset: int, need: int) -> np.ndarray:
    """contiguous uint8 view of bytes / an array, checked to hold `need` bytes from `offset` on (never empty: ctypes wants an address)"""
    buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    assert buf.size >= offset + need, "short input"
    return buf if buf.size else np.zeros(1, dtype=np.uint8)


def _addr(buf: np.ndarray, offset: int):
    return C.c_void_p(buf.ctypes.data + offset)


def _proof_tuple(curve: int, proof: "G16ProofC"):
    nq = FQ_LIMBS[curve]
    return (np.array(proof.a[: 2 * nq], dtype=np.uint64), proof.a_inf, np.array(proof.b[: 4 * nq], dtype=np.uint64), proof.b_inf,
            np.array(proof.c[: 2 * nq], dtype=np.uint64), proof.c_inf)


class Backend:
    """One zl_ctx (one GPU, one stream).  Mirrors the two upstream entry points the arkworks plugin surfaces:
    VariableBaseMSM::multi_scalar_mul -> msm(); Radix2EvaluationDomain::{fft,ifft,coset_*} -> ntt()."""

    def __init__(self, device: int = 0, _borrowed_ctx=None):
        self.L = load_library()
        self._bases = {}
        self._owned = _borrowed_ctx is None
        if _borrowed_ctx is not None:  # a rank of a MultiBackend: the zl_mctx owns the ctx
            self._ctx = C.c_void_p(_borrowed_ctx)
            return
        self._ctx = C.c_void_p()
        self._check(self.L.zl_ctx_create(C.byref(self._ctx), device), "zl_ctx_create")

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise BackendError(rc, what, self.L.zl_strerror(rc).decode())

    def fork(self) -> "Backend":
        """zl_ctx_fork: a second prover lane on this device that reads this backend's device-resident keys (one lane per host thread; close it before this one)"""
        child = Backend.__new__(Backend)
        child.L, child._bases, child._owned, child._parent = self.L, collections.ChainMap({}, self._bases), True, self
        child._ctx = C.c_void_p()
        self._check(self.L.zl_ctx_fork(self._ctx, C.byref(child._ctx)), "zl_ctx_fork")
        self.__dict__.setdefault("_forks", []).append(child)
        return child

    def close(self):
        for f in self.__dict__.pop("_forks", []):  # the lanes go first: they read this ctx's objects
            f.close()
        if self._ctx:
            if self._owned:
                self.L.zl_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def pairing_product(self, curve: int, ps: np.ndarray, qs: np.ndarray) -> np.ndarray:
        """prod_i e(P_i, Q_i) (ark's product_of_pairings) as 12 canonical Fq coefficients: device Miller loops, one host final exponentiation.
        ps: (n, 2 FQ64) G1 points x||y, qs: (n, 4 FQ64) G2 points x.c0||x.c1||y.c0||y.c1, canonical u64 words; all-zero = infinity."""
        nq = FQ_LIMBS[curve]
        p = np.ascontiguousarray(np.asarray(ps, dtype=np.uint64).reshape(-1, 2 * nq))
        q = np.ascontiguousarray(np.asarray(qs, dtype=np.uint64).reshape(-1, 4 * nq))
        assert p.shape[0] == q.shape[0]
        n = p.shape[0]
        if n == 0:
            p, q = np.zeros((1, 2 * nq), dtype=np.uint64), np.zeros((1, 4 * nq), dtype=np.uint64)
        out = np.zeros((12, nq), dtype=np.uint64)
        self._check(self.L.zl_pairing_product(self._ctx, curve, _p64(p), _p64(q), n, _p64(out)), "zl_pairing_product")
        return out

    def pairing_products(self, curve: int, ps: np.ndarray, qs: np.ndarray, pairs_each: int, count: Optional[int] = None):
        """zl_pairing_products: `count` independent products of `pairs_each` pairings, Miller loops and final exponentiations on the device.  ps / qs as
        pairing_product, product j over pairs [j pairs_each, (j + 1) pairs_each); count defaults to what ps holds.  Returns (values (count, 12, FQ64) canonical
        words -- row j is pairing_product of product j's pairs --, status (count,) int32: 0 or ZL_ENOTCURVE for a zero Miller product)."""
        nq = FQ_LIMBS[curve]
        p = np.ascontiguousarray(np.asarray(ps, dtype=np.uint64).reshape(-1, 2 * nq))
        q = np.ascontiguousarray(np.asarray(qs, dtype=np.uint64).reshape(-1, 4 * nq))
        if count is None:
            count = p.shape[0] // pairs_each if pairs_each else 0
        assert p.shape[0] == q.shape[0] and p.shape[0] >= count * pairs_each
        if p.shape[0] == 0:
            p, q = np.zeros((1, 2 * nq), dtype=np.uint64), np.zeros((1, 4 * nq), dtype=np.uint64)
        out = np.zeros((max(1, count), 12, nq), dtype=np.uint64)
        status = np.zeros(max(1, count), dtype=np.int32)
        self._check(self.L.zl_pairing_products(self._ctx, curve, _p64(p), _p64(q), count, pairs_each, _p64(out), status.ctypes.data_as(i32p)), "zl_pairing_products")
        return out[:count], status[:count]

    def points_from_bytes(self, curve: int, group: int, data, count: int, offset: int = 0):
        """zl_points_from_bytes_batch: `count` compressed points decoded on the device (square roots, sign rule, subgroup check), one lane per point.
        data: bytes or a uint8 array holding the packed records from byte `offset` on (any alignment).  Returns (xy (count, 2 or 4 x FQ64) canonical words,
        inf (count,) uint8, status (count,) int32): per record what point_from_bytes gives -- a bad record is a status, not an exception."""
        rec = self.L.zl_point_bytes(curve, group)
        buf = _bytes_view(data, offset, count * rec)
        xy = np.zeros((count, 2 * group * FQ_LIMBS[curve]), dtype=np.uint64)
        inf = np.zeros(count, dtype=np.uint8)
        st = np.zeros(count, dtype=np.int32)
        self._check(self.L.zl_points_from_bytes_batch(self._ctx, curve, group, _addr(buf, offset), count, _p64(xy) if count else None, inf.ctypes.data_as(u8p) if count else None,
                                                      st.ctypes.data_as(i32p) if count else None), "zl_points_from_bytes_batch")
        return xy, inf, st

    def proofs_from_bytes(self, curve: int, data, count: int):
        """zl_groth16_proofs_from_bytes_batch: `count` wire proofs decoded on the device -> (proof tuples as proof_from_bytes returns them, status (count,) int32).
        A record whose status is not 0 did not decode (its tuple holds what the host decoder leaves: the points in front of the failing one)."""
        buf = _bytes_view(data, 0, count * self.L.zl_groth16_proof_bytes(curve))
        out = (G16ProofC * max(1, count))()
        st = np.zeros(max(1, count), dtype=np.int32)
        self._check(self.L.zl_groth16_proofs_from_bytes_batch(self._ctx, curve, _addr(buf, 0), count, out, st.ctypes.data_as(i32p)), "zl_groth16_proofs_from_bytes_batch")
        return [_proof_tuple(curve, p) for p in out[:count]], st[:count]

    def describe(self) -> str:
        buf = C.create_string_buffer(512)
        self.L.zl_describe(self._ctx, buf, 512)
        return buf.value.decode()

    def set_stream(self, stream_handle: int):
        self._check(self.L.zl_ctx_set_stream(self._ctx, C.c_void_p(stream_handle)), "zl_ctx_set_stream")

    def set_msm_window(self, c: int):
        self._check(self.L.zl_ctx_set_msm_window(self._ctx, c), "zl_ctx_set_msm_window")

    def enable_timing(self, on: bool = True):
        self._check(self.L.zl_ctx_enable_timing(self._ctx, int(on)), "zl_ctx_enable_timing")

    def last_timing(self) -> Timing:
        t = Timing()
        self._check(self.L.zl_last_timing(self._ctx, C.byref(t)), "zl_last_timing")
        return t

    def sync(self):
        self._check(self.L.zl_ctx_sync(self._ctx), "zl_ctx_sync")

    # ---- bases ------------------------------------------------------------------------------------------------
    def bases_upload(self, curve: int, xy: np.ndarray, group: int = ZL_G1, flags: int = 0, stride: int = 0, inf_offset: int = -1,
                     n: Optional[int] = None) -> int:
        h = C.c_uint64()
        if n is None:
            n = xy.shape[0]
        ptr = xy.ctypes.data_as(C.c_void_p) if xy.size else None
        self._check(self.L.zl_bases_upload(self._ctx, curve, group, ptr, n, stride, inf_offset, flags, C.byref(h)), "zl_bases_upload")
        self._bases[h.value] = (curve, group, n)
        return h.value

    def bases_generate(self, curve: int, k: np.ndarray, group: int = ZL_G1) -> int:
        h = C.c_uint64()
        self._check(self.L.zl_bases_generate(self._ctx, curve, group, _p64(k), k.shape[0], C.byref(h)), "zl_bases_generate")
        self._bases[h.value] = (curve, group, k.shape[0])
        return h.value

    def bases_download(self, handle: int, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        curve, group, n = self._bases[handle]
        if count is None:
            count = n - first
        out = np.zeros((count, 2 * group * FQ_LIMBS[curve]), dtype=np.uint64)
        self._check(self.L.zl_bases_download(self._ctx, handle, first, count, _p64(out)), "zl_bases_download")
        return out

    def bases_precompute(self, handle: int, c: int = 0):
        """build the table of 2^(c w) P_i (W x memory) so that all windows share one bucket set"""
        self._check(self.L.zl_bases_precompute(self._ctx, handle, c), "zl_bases_precompute")

    def bases_free(self, handle: int):
        self._check(self.L.zl_bases_free(self._ctx, handle), "zl_bases_free")
        self._bases.pop(handle, None)

    # ---- MSM --------------------------------------------------------------------------------------------------
    def _out(self, handle: int):
        curve, group, _ = self._bases[handle]
        return np.zeros(2 * group * FQ_LIMBS[curve], dtype=np.uint64)

    def msm(self, handle: int, scalars: np.ndarray, first: int = 0) -> Tuple[np.ndarray, int]:
        """scalars: (n,4) uint64 canonical, host memory."""
        out, inf = self._out(handle), C.c_uint8(0)
        n = scalars.shape[0]
        self._check(self.L.zl_msm(self._ctx, handle, first, _p64(scalars) if n else None, n, _p64(out), C.byref(inf)), "zl_msm")
        return out, inf.value

    def msm_dev(self, handle: int, d_scalars: int, n: int, first: int = 0) -> Tuple[np.ndarray, int]:
        """d_scalars: device pointer (e.g. torch tensor .data_ptr()) to n x 4 u64 canonical scalars in HBM."""
        out, inf = self._out(handle), C.c_uint8(0)
        self._check(self.L.zl_msm_dev(self._ctx, handle, first, C.c_void_p(d_scalars), n, _p64(out), C.byref(inf)), "zl_msm_dev")
        return out, inf.value

    def msm_partial_dev(self, handle: int, d_scalars: int, n: int, first: int = 0) -> np.ndarray:
        out = np.zeros(ZL_PARTIAL_WORDS, dtype=np.uint64)
        self._check(self.L.zl_msm_partial_dev(self._ctx, handle, first, C.c_void_p(d_scalars), n, _p64(out)), "zl_msm_partial_dev")
        return out

    def msm_batch_partial_dev(self, handle: int, d_scalars, n: int, first: int = 0) -> np.ndarray:
        """d_scalars: list of device pointers (one scalar vector per MSM) -> (count, ZL_PARTIAL_WORDS) partial sums; pipelined."""
        count = len(d_scalars)
        ptrs = (C.c_void_p * max(1, count))(*[int(p) for p in d_scalars])
        out = np.zeros((count, ZL_PARTIAL_WORDS), dtype=np.uint64)
        self._check(self.L.zl_msm_batch_partial_dev(self._ctx, handle, first, ptrs, n, count, _p64(out)), "zl_msm_batch_partial_dev")
        return out

    def msm_multi_dev(self, handle: int, d_scalars: int, n: int, count: int, stride: Optional[int] = None, first: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """`count` MSMs over bases [first, first + n) in one device pass: vector j = n x 4 u64 canonical scalars at d_scalars + j * stride * 32 bytes
        (stride in scalars, default n) -> ((count, words) canonical affine results, (count,) infinity flags), each row what msm_dev gives for that vector."""
        curve, group, _ = self._bases[handle]
        out = np.zeros((count, 2 * group * FQ_LIMBS[curve]), dtype=np.uint64)
        inf = np.zeros(max(1, count), dtype=np.uint8)
        self._check(self.L.zl_msm_multi_dev(self._ctx, handle, first, C.c_void_p(d_scalars), n, n if stride is None else stride, count, _p64(out) if count else None,
                                            inf.ctypes.data_as(u8p)), "zl_msm_multi_dev")
        return out, inf[:count]

    def partials_sum(self, curve: int, partials: np.ndarray, group: int = ZL_G1) -> Tuple[np.ndarray, int]:
        partials = np.ascontiguousarray(partials.reshape(-1, ZL_PARTIAL_WORDS))
        out, inf = np.zeros(2 * group * FQ_LIMBS[curve], dtype=np.uint64), C.c_uint8(0)
        self._check(self.L.zl_partials_sum(curve, group, _p64(partials), partials.shape[0], _p64(out), C.byref(inf)), "zl_partials_sum")
        return out, inf.value

    # ---- NTT --------------------------------------------------------------------------------------------------
    def ntt(self, curve: int, data: np.ndarray, inverse: bool = False, coset: bool = False, mont: bool = False) -> np.ndarray:
        """data: (2^k, 4) uint64, returns the transformed copy (natural order)."""
        d = np.ascontiguousarray(data.copy())
        n = d.shape[0]
        log_n = n.bit_length() - 1
        if n == 0 or (1 << log_n) != n:
            raise BackendError(-1, "zl_ntt", "length must be a power of two")
        flags = (ZL_INVERSE if inverse else 0) | (ZL_COSET if coset else 0) | (ZL_MONT if mont else 0)
        self._check(self.L.zl_ntt(self._ctx, curve, _p64(d), log_n, flags), "zl_ntt")
        return d

    def ntt_dev(self, curve: int, d_data: int, log_n: int, inverse: bool = False, coset: bool = False, mont: bool = True):
        flags = (ZL_INVERSE if inverse else 0) | (ZL_COSET if coset else 0) | (ZL_MONT if mont else 0)
        self._check(self.L.zl_ntt_dev(self._ctx, curve, C.c_void_p(d_data), log_n, flags), "zl_ntt_dev")

    def ntt_dev_flags(self, curve: int, d_data: int, log_n: int, flags: int):
        """zl_ntt_dev with raw flags (ZL_MONT_IN / ZL_MONT_OUT legs of the distributed transform)."""
        self._check(self.L.zl_ntt_dev(self._ctx, curve, C.c_void_p(d_data), log_n, flags), "zl_ntt_dev")

    def ntt_batch_dev(self, curve: int, d_data: int, log_n: int, flags: int, count: int, stride_elems: int):
        """`count` equal transforms, one launch per pass (include/zl_backend_ext.h: zl_ntt_batch_dev)."""
        self._check(self.L.zl_ntt_batch_dev(self._ctx, curve, C.c_void_p(d_data), log_n, flags, count, stride_elems), "zl_ntt_batch_dev")

    def ntt_cross_dev(self, curve: int, d_data: int, log_n: int, log_g: int, rank: int, flags: int):
        """Cross-rank step of the distributed transform (include/zl_backend.h: zl_ntt_cross_dev)."""
        self._check(self.L.zl_ntt_cross_dev(self._ctx, curve, C.c_void_p(d_data), log_n, log_g, rank, flags), "zl_ntt_cross_dev")

    # ---- batched Poseidon (include/zl_backend_ext.h; the module-level poseidon_*_host functions are the same calls with ctx == NULL) ----------
    def poseidon_permute_batch(self, curve: int, states: np.ndarray) -> np.ndarray:
        """(count, W, 4) canonical states, W in 3..6 -> the permuted copy (zl_poseidon_permute_batch / _w); any other shape is taken as width-3 states"""
        return _poseidon_permute_batch(self.L, self._ctx, curve, states)

    def poseidon_hash(self, curve: int, inputs: np.ndarray) -> np.ndarray:
        """(count, arity, 4) canonical inputs, arity in 2..5 -> (count, 4) digests: element 0 of permute([2^arity - 1, x_1 .. x_arity]) (zl_poseidon_hash_batch)"""
        return _poseidon_hash(self.L, self._ctx, curve, inputs)

    def poseidon_hash_dev(self, curve: int, arity: int, d_in: int, count: int, d_out: int):
        """zl_poseidon_hash_batch_dev: count x arity elements at device address d_in -> count digests at d_out; finished on return"""
        self._check(self.L.zl_poseidon_hash_batch_dev(self._ctx, curve, arity, C.c_void_p(d_in), count, C.c_void_p(d_out)), "zl_poseidon_hash_batch_dev")

    def poseidon_duplex_encrypt(self, curve: int, initial_state, keys, headers, plaintexts):
        """the duplex cipher (zl_poseidon_duplex_encrypt_batch): plaintexts (count, N, W - 1, 4) -- which fixes the width W --, keys (count, K, 4), headers
        (count, H, 4), initial_state (W, 4) or None (zero) -> (ciphertexts shaped as plaintexts, tags (count, 4))"""
        return _poseidon_duplex(self.L, self._ctx, curve, initial_state, keys, headers, plaintexts, None)

    def poseidon_duplex_decrypt(self, curve: int, initial_state, keys, headers, ciphertexts, tags):
        """zl_poseidon_duplex_decrypt_batch -> (plaintexts, ok): ok[i] is whether tags[i] is the tag of item i; the plaintexts are returned either way"""
        return _poseidon_duplex(self.L, self._ctx, curve, initial_state, keys, headers, ciphertexts, tags)

    def poseidon_duplex_encrypt_dev(self, curve: int, width: int, initial_state, d_keys: int, key_len: int, d_headers: int, header_len: int, d_plaintexts: int,
                                    blocks: int, count: int, d_ciphertexts: int, d_tags: int):
        """zl_poseidon_duplex_encrypt_batch_dev on device addresses (d_ciphertexts may be d_plaintexts); initial_state stays host memory; finished on return"""
        st = _duplex_state(initial_state, width)
        self._check(self.L.zl_poseidon_duplex_encrypt_batch_dev(self._ctx, curve, width, None if st is None else _p64(st), C.c_void_p(d_keys), key_len,
                                                                C.c_void_p(d_headers), header_len, C.c_void_p(d_plaintexts), blocks, count, C.c_void_p(d_ciphertexts),
                                                                C.c_void_p(d_tags)), "zl_poseidon_duplex_encrypt_batch_dev")

    def poseidon_duplex_decrypt_dev(self, curve: int, width: int, initial_state, d_keys: int, key_len: int, d_headers: int, header_len: int, d_ciphertexts: int,
                                    d_tags: int, blocks: int, count: int, d_plaintexts: int) -> np.ndarray:
        """zl_poseidon_duplex_decrypt_batch_dev on device addresses -> the (count,) bool verdicts (host memory)"""
        st = _duplex_state(initial_state, width)
        ok = np.zeros(count, dtype=np.uint8)
        self._check(self.L.zl_poseidon_duplex_decrypt_batch_dev(self._ctx, curve, width, None if st is None else _p64(st), C.c_void_p(d_keys), key_len,
                                                                C.c_void_p(d_headers), header_len, C.c_void_p(d_ciphertexts), C.c_void_p(d_tags), blocks, count,
                                                                C.c_void_p(d_plaintexts), ok.ctypes.data_as(C.POINTER(C.c_uint8)) if count else None),
                    "zl_poseidon_duplex_decrypt_batch_dev")
        return ok.astype(bool)

    def ed_scalar_mul(self, curve: int, points, scalars, check_subgroup: bool = False):
        """zl_ed_scalar_mul_batch on the embedded curve of `curve`: points (count, 2, 4) or one point (2, 4), scalars (count, 4) or one scalar (4,) -- a single
        operand broadcasts through stride 0 -> (out (count, 2, 4), status (count,) uint8: 0 ok, 1 coordinate >= q, 2 off the curve, 3 outside the subgroup (with
        check_subgroup), 4 scalar >= l; a refused item is (0, 1))"""
        return _ed_scalar_mul(self.L, self._ctx, curve, points, scalars, check_subgroup)

    def ed_scalar_mul_dev(self, curve: int, d_points: int, point_stride: int, d_scalars: int, scalar_stride: int, count: int, d_out: int, d_status: int,
                          check_subgroup: bool = False):
        """zl_ed_scalar_mul_batch_dev on device addresses (d_status may be 0: a refused item then fails the call); finished on return"""
        self._check(self.L.zl_ed_scalar_mul_batch_dev(self._ctx, curve, C.c_void_p(d_points), point_stride, C.c_void_p(d_scalars), scalar_stride, count,
                                                      ZL_ED_CHECK_SUBGROUP if check_subgroup else 0, C.c_void_p(d_out), C.c_void_p(d_status)), "zl_ed_scalar_mul_batch_dev")

    def ed_scalar_mul_assignments(self, curve: int, points, scalars, bits: Optional[int] = None) -> np.ndarray:
        """zl_ed_scalar_mul_assignments: points (count, 2, 4) or one point (2, 4), scalars (count, 4) -> (count, ed_scalar_mul_assignment_elems(curve, bits), 4)
        canonical words, row i the complete assignment of Circuit.ed_scalar_mul(curve, points[i], scalars[i], bits); bits None: the full width of the curve"""
        return _ed_scalar_mul_assignments(self.L, self._ctx, curve, points, scalars, bits)

    def ed_scalar_mul_assignments_dev(self, curve: int, bits: int, d_points: int, point_stride: int, d_scalars: int, count: int, d_out: int,
                                      stride_elems: Optional[int] = None):
        """zl_ed_scalar_mul_assignments_dev on device addresses -> row i at d_out + i * stride_elems elements (default: the row length); finished on return"""
        stride = self.L.zl_ed_scalar_mul_assignment_elems(curve, bits) if stride_elems is None else stride_elems
        self._check(self.L.zl_ed_scalar_mul_assignments_dev(self._ctx, curve, bits, C.c_void_p(d_points), point_stride, C.c_void_p(d_scalars), count, C.c_void_p(d_out),
                                                            stride), "zl_ed_scalar_mul_assignments_dev")

    def _prove_scalar_muls(self, pkc, curve: int, r1cs_handle: int, bits: int, points, scalars, r: np.ndarray, s: np.ndarray):
        (p, ps), k = _ed_operand(points, 2, "points"), np.ascontiguousarray(np.asarray(scalars, dtype=np.uint64)).reshape(-1, 4)
        count = k.shape[0]
        if ps and p.shape[0] != count:
            raise ValueError("operands of different counts")
        r, s = np.ascontiguousarray(r, dtype=np.uint64).reshape(count, 4), np.ascontiguousarray(s, dtype=np.uint64).reshape(count, 4)
        out = (G16ProofC * max(1, count))()
        q = np.zeros((count, 2, 4), dtype=np.uint64)
        self._check(self.L.zl_groth16_prove_ed_scalar_muls(self._ctx, C.byref(pkc), r1cs_handle, bits, _p64(p), ps, _ptr_or_none(k), _ptr_or_none(r), _ptr_or_none(s), count,
                                                           out, _ptr_or_none(q)), "zl_groth16_prove_ed_scalar_muls")
        return [_proof_tuple(curve, pr) for pr in out[:count]], q

    def groth16_prove_ed_scalar_muls(self, curve: int, pk: dict, r1cs_handle: int, bits: int, points, scalars, r: np.ndarray, s: np.ndarray):
        """zl_groth16_prove_ed_scalar_muls: points (count, 2, 4) or one (2, 4), scalars (count, 4) and blinding scalars -> (`count` proofs, Q (count, 2, 4)): the
        public inputs of proof j are points[j] and Q[j]"""
        pkc, keep_pk = _pk_struct(curve, pk)
        return self._prove_scalar_muls(pkc, curve, r1cs_handle, bits, points, scalars, r, s)

    def hybrid_encrypt_assignments(self, curve: int, initial_state, generator, esk, pks, headers, plaintexts, bits: Optional[int] = None) -> np.ndarray:
        """zl_hybrid_encrypt_assignments: operands as hybrid_encrypt -> (count, hybrid_encrypt_assignment_elems(curve, W, bits, H, N), 4) canonical words, row i the
        complete assignment of Circuit.hybrid_encrypt(curve, initial_state, generator, esk[i], pks[i], headers[i], plaintexts[i], bits); bits None: the full width"""
        return _hybrid_encrypt_assignments(self.L, self._ctx, curve, initial_state, generator, esk, pks, headers, plaintexts, bits)

    def hybrid_encrypt_assignments_dev(self, curve: int, width: int, bits: int, initial_state, generator, d_esk: int, d_pks: int, pk_stride: int, d_headers: int,
                                       header_len: int, d_plaintexts: int, blocks: int, count: int, d_out: int, stride_elems: Optional[int] = None):
        """zl_hybrid_encrypt_assignments_dev on device addresses -> row i at d_out + i * stride_elems elements (default: the row length); generator and
        initial_state stay host memory; finished on return"""
        st = _duplex_state(initial_state, width)
        g = np.ascontiguousarray(np.asarray(generator, dtype=np.uint64).reshape(2, 4))
        stride = self.L.zl_hybrid_encrypt_assignment_elems(curve, width, bits, header_len, blocks) if stride_elems is None else stride_elems
        self._check(self.L.zl_hybrid_encrypt_assignments_dev(self._ctx, curve, width, bits, None if st is None else _p64(st), _p64(g), C.c_void_p(d_esk), C.c_void_p(d_pks),
                                                             pk_stride, C.c_void_p(d_headers), header_len, C.c_void_p(d_plaintexts), blocks, count, C.c_void_p(d_out), stride),
                    "zl_hybrid_encrypt_assignments_dev")

    def _prove_hybrid_encryptions(self, pkc, curve: int, r1cs_handle: int, bits: int, initial_state, generator, esk, pks, headers, plaintexts, r: np.ndarray, s: np.ndarray):
        st, g, e, pk, ps, h, t = _hybrid_operands(initial_state, generator, esk, pks, headers, plaintexts)
        count, blocks, width = t.shape[0], t.shape[1], t.shape[2] + 1
        r, s = np.ascontiguousarray(r, dtype=np.uint64).reshape(count, 4), np.ascontiguousarray(s, dtype=np.uint64).reshape(count, 4)
        out = (G16ProofC * max(1, count))()
        epks, tags, cts = np.zeros((count, 2, 4), dtype=np.uint64), np.zeros((count, 4), dtype=np.uint64), np.zeros_like(t)
        self._check(self.L.zl_groth16_prove_hybrid_encryptions(self._ctx, C.byref(pkc), r1cs_handle, width, bits, None if st is None else _p64(st), _p64(g), _ptr_or_none(e),
                                                               _p64(pk), ps, _ptr_or_none(h), h.shape[1], _ptr_or_none(t), blocks, _ptr_or_none(r), _ptr_or_none(s), count, out,
                                                               _ptr_or_none(epks), _ptr_or_none(tags), _ptr_or_none(cts)), "zl_groth16_prove_hybrid_encryptions")
        return [_proof_tuple(curve, p) for p in out[:count]], epks, tags, cts

    def groth16_prove_hybrid_encryptions(self, curve: int, pk: dict, r1cs_handle: int, bits: int, initial_state, generator, esk, pks, headers, plaintexts, r: np.ndarray,
                                         s: np.ndarray):
        """zl_groth16_prove_hybrid_encryptions: operands as hybrid_encrypt and blinding scalars -> (`count` proofs, epks (count, 2, 4), tags (count, 4), ciphertexts):
        the public inputs of proof j are the generator, pks[j], epks[j], tags[j], ciphertexts[j] and headers[j]"""
        pkc, keep_pk = _pk_struct(curve, pk)
        return self._prove_hybrid_encryptions(pkc, curve, r1cs_handle, bits, initial_state, generator, esk, pks, headers, plaintexts, r, s)

    def hybrid_encrypt(self, curve: int, initial_state, generator, esk, pks, headers, plaintexts, check_subgroup: bool = False):
        """zl_hybrid_encrypt_batch: generator (2, 4), esk (count, 4), pks (count, 2, 4) or one (2, 4), headers (count, H, 4), plaintexts (count, N, W - 1, 4) ->
        (epks (count, 2, 4), ciphertexts, tags (count, 4), status (count,)): epk = esk G, the duplex cipher under the key (x, y) of esk pk"""
        return _hybrid_encrypt(self.L, self._ctx, curve, initial_state, generator, esk, pks, headers, plaintexts, check_subgroup)

    def hybrid_decrypt(self, curve: int, initial_state, sks, epks, headers, ciphertexts, tags, check_subgroup: bool = False):
        """zl_hybrid_decrypt_batch: sks (count, 4) or ONE key (4,) -- the scan --, epks (count, 2, 4) -> (plaintexts, ok (count,) bool, status (count,)): the key
        is (x, y) of sk epk; ok[i] is False for a tag mismatch and for a refused point"""
        return _hybrid_decrypt(self.L, self._ctx, curve, initial_state, sks, epks, headers, ciphertexts, tags, check_subgroup)

    def hybrid_encrypt_dev(self, curve: int, width: int, initial_state, generator, d_esk: int, d_pks: int, pk_stride: int, d_headers: int, header_len: int,
                           d_plaintexts: int, blocks: int, count: int, d_epks: int, d_ciphertexts: int, d_tags: int, d_status: int, check_subgroup: bool = False):
        """zl_hybrid_encrypt_batch_dev on device addresses; generator and initial_state stay host memory; finished on return"""
        st = _duplex_state(initial_state, width)
        g = np.ascontiguousarray(np.asarray(generator, dtype=np.uint64).reshape(2, 4))
        self._check(self.L.zl_hybrid_encrypt_batch_dev(self._ctx, curve, width, None if st is None else _p64(st), _p64(g), C.c_void_p(d_esk), C.c_void_p(d_pks), pk_stride,
                                                       C.c_void_p(d_headers), header_len, C.c_void_p(d_plaintexts), blocks, count,
                                                       ZL_ED_CHECK_SUBGROUP if check_subgroup else 0, C.c_void_p(d_epks), C.c_void_p(d_ciphertexts), C.c_void_p(d_tags),
                                                       C.c_void_p(d_status)), "zl_hybrid_encrypt_batch_dev")

    def hybrid_decrypt_dev(self, curve: int, width: int, initial_state, d_sks: int, sk_stride: int, d_epks: int, d_headers: int, header_len: int, d_ciphertexts: int,
                           d_tags: int, blocks: int, count: int, d_plaintexts: int, d_status: int, check_subgroup: bool = False) -> np.ndarray:
        """zl_hybrid_decrypt_batch_dev on device addresses -> the (count,) bool verdicts (host memory)"""
        st = _duplex_state(initial_state, width)
        ok = np.zeros(count, dtype=np.uint8)
        self._check(self.L.zl_hybrid_decrypt_batch_dev(self._ctx, curve, width, None if st is None else _p64(st), C.c_void_p(d_sks), sk_stride, C.c_void_p(d_epks),
                                                       C.c_void_p(d_headers), header_len, C.c_void_p(d_ciphertexts), C.c_void_p(d_tags), blocks, count,
                                                       ZL_ED_CHECK_SUBGROUP if check_subgroup else 0, C.c_void_p(d_plaintexts),
                                                       ok.ctypes.data_as(C.POINTER(C.c_uint8)) if count else None, C.c_void_p(d_status)), "zl_hybrid_decrypt_batch_dev")
        return ok.astype(bool)

    def poseidon_hash2(self, curve: int, xy: np.ndarray) -> np.ndarray:
        """(count, 2, 4) canonical pairs -> (count, 4) digests H(x, y)"""
        return _poseidon_hash2(self.L, self._ctx, curve, xy)

    def poseidon_hash2_dev(self, curve: int, d_xy: int, count: int, d_out: int):
        """zl_poseidon_hash2_batch_dev: count pairs at device address d_xy -> count digests at d_out; finished on return"""
        self._check(self.L.zl_poseidon_hash2_batch_dev(self._ctx, curve, C.c_void_p(d_xy), count, C.c_void_p(d_out)), "zl_poseidon_hash2_batch_dev")

    def poseidon_chain(self, curve: int, x0: np.ndarray, x1: np.ndarray, k: int) -> np.ndarray:
        """out[i] = h_k of the chain over (x0[i], x1[i]): the public input of Circuit(curve, k, x0[i], x1[i])"""
        return _poseidon_chain(self.L, self._ctx, curve, x0, x1, k)

    def poseidon_chain_assignments(self, curve: int, x0: np.ndarray, x1: np.ndarray, k: int) -> np.ndarray:
        """zl_poseidon_chain_assignments: (count, 4 + 234 k, 4) canonical words, row i the complete assignment of Circuit(curve, k, x0[i], x1[i])"""
        return _poseidon_chain_assignments(self.L, self._ctx, curve, x0, x1, k)

    def poseidon_chain_assignments_dev(self, curve: int, d_x0: int, d_x1: int, k: int, count: int, d_out: int, stride_elems: Optional[int] = None):
        """zl_poseidon_chain_assignments_dev: count chains from the device addresses d_x0 / d_x1 -> row i at d_out + i * stride_elems elements (default: the
        row length, poseidon_chain_assignment_elems(k)); finished on return"""
        stride = self.L.zl_poseidon_chain_assignment_elems(k) if stride_elems is None else stride_elems
        self._check(self.L.zl_poseidon_chain_assignments_dev(self._ctx, curve, C.c_void_p(d_x0), C.c_void_p(d_x1), k, count, C.c_void_p(d_out), stride),
                    "zl_poseidon_chain_assignments_dev")

    def poseidon_merkle_root(self, curve: int, leaves: np.ndarray, depth: int) -> np.ndarray:
        return _poseidon_merkle_root(self.L, self._ctx, curve, leaves, depth)

    def poseidon_merkle_build(self, curve: int, leaves: np.ndarray, depth: int):
        """host leaves -> (nodes (zl_poseidon_merkle_nodes, 4), root (4,))"""
        return _poseidon_merkle_build(self.L, self._ctx, curve, leaves, depth)

    def poseidon_merkle_build_dev(self, curve: int, d_leaves: int, n: int, depth: int, d_nodes: int) -> np.ndarray:
        """zl_poseidon_merkle_build_dev: every level into the device node array at d_nodes (poseidon_merkle_nodes(n, depth) elements); returns the root"""
        root = np.zeros(4, dtype=np.uint64)
        self._check(self.L.zl_poseidon_merkle_build_dev(self._ctx, curve, C.c_void_p(d_leaves), n, depth, C.c_void_p(d_nodes), _p64(root)), "zl_poseidon_merkle_build_dev")
        return root

    def poseidon_merkle_paths(self, curve: int, d_nodes: int, n: int, depth: int, indices) -> np.ndarray:
        """(count, depth, 4) sibling digests of the leaves `indices`, bottom up, gathered from the device node array"""
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        paths = np.zeros((max(1, idx.size), depth, 4), dtype=np.uint64)
        self._check(self.L.zl_poseidon_merkle_paths_dev(self._ctx, curve, C.c_void_p(d_nodes), n, depth, _p64(idx) if idx.size else None, idx.size, _p64(paths)),
                    "zl_poseidon_merkle_paths_dev")
        return paths[: idx.size]

    def poseidon_merkle_roots_from_paths(self, curve: int, leaves: np.ndarray, indices, paths: np.ndarray, depth: int) -> np.ndarray:
        return _poseidon_roots_from_paths(self.L, self._ctx, curve, leaves, indices, paths, depth)

    def poseidon_merkle_assignments(self, curve: int, leaves, indices, paths, depth: int) -> np.ndarray:
        """zl_poseidon_merkle_assignments: (count, 3 + 238 depth, 4) canonical words, row i the complete assignment of
        Circuit.merkle(curve, depth, leaves[i], indices[i], paths[i])"""
        return _poseidon_merkle_assignments(self.L, self._ctx, curve, leaves, indices, paths, depth)

    def poseidon_merkle_assignments_dev(self, curve: int, d_leaves: int, indices, d_paths: int, depth: int, d_out: int, stride_elems: Optional[int] = None):
        """zl_poseidon_merkle_assignments_dev: leaves and paths at device addresses, indices in host memory -> row i at d_out + i * stride_elems elements
        (default: the row length, poseidon_merkle_assignment_elems(depth)); finished on return"""
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        stride = self.L.zl_poseidon_merkle_assignment_elems(depth) if stride_elems is None else stride_elems
        self._check(self.L.zl_poseidon_merkle_assignments_dev(self._ctx, curve, C.c_void_p(d_leaves), _ptr_or_none(idx), C.c_void_p(d_paths), depth, idx.size,
                                                              C.c_void_p(d_out), stride), "zl_poseidon_merkle_assignments_dev")

    def poseidon_merkle_member_assignments_dev(self, curve: int, d_nodes: int, n: int, depth: int, indices, d_out: int, stride_elems: Optional[int] = None):
        """zl_poseidon_merkle_member_assignments_dev: the memberships of the leaves `indices` (host memory) of the tree at the device address d_nodes
        (poseidon_merkle_build_dev's node array) -> rows as poseidon_merkle_assignments_dev"""
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        stride = self.L.zl_poseidon_merkle_assignment_elems(depth) if stride_elems is None else stride_elems
        self._check(self.L.zl_poseidon_merkle_member_assignments_dev(self._ctx, curve, C.c_void_p(d_nodes), n, depth, _ptr_or_none(idx), idx.size, C.c_void_p(d_out),
                                                                     stride), "zl_poseidon_merkle_member_assignments_dev")

    def poseidon_encrypt_assignments(self, curve: int, initial_state, keys, headers, plaintexts) -> np.ndarray:
        """zl_poseidon_encrypt_assignments: operands as poseidon_duplex_encrypt (keys (count, K, 4) with K >= 1) -> (count, poseidon_encrypt_assignment_elems(W, K,
        H, N), 4) canonical words, row i the complete assignment of Circuit.poseidon_encrypt(curve, initial_state, keys[i], headers[i], plaintexts[i])"""
        return _poseidon_encrypt_assignments(self.L, self._ctx, curve, initial_state, keys, headers, plaintexts)

    def poseidon_encrypt_assignments_dev(self, curve: int, width: int, initial_state, d_keys: int, key_len: int, d_headers: int, header_len: int, d_plaintexts: int,
                                         blocks: int, count: int, d_out: int, stride_elems: Optional[int] = None):
        """zl_poseidon_encrypt_assignments_dev on device addresses -> row i at d_out + i * stride_elems elements (default: the row length); initial_state stays
        host memory; finished on return"""
        st = _duplex_state(initial_state, width)
        stride = self.L.zl_poseidon_encrypt_assignment_elems(width, key_len, header_len, blocks) if stride_elems is None else stride_elems
        self._check(self.L.zl_poseidon_encrypt_assignments_dev(self._ctx, curve, width, None if st is None else _p64(st), C.c_void_p(d_keys), key_len,
                                                               C.c_void_p(d_headers), header_len, C.c_void_p(d_plaintexts), blocks, count, C.c_void_p(d_out), stride),
                    "zl_poseidon_encrypt_assignments_dev")

    def poseidon_hash_assignments(self, curve: int, inputs) -> np.ndarray:
        """zl_poseidon_hash_assignments: inputs (count, arity, 4) -> (count, 2 + arity + 3 S(arity), 4) canonical words, row i the complete assignment of
        Circuit.poseidon_hash(curve, inputs[i])"""
        return _poseidon_hash_assignments(self.L, self._ctx, curve, inputs)

    def poseidon_hash_assignments_dev(self, curve: int, arity: int, d_in: int, count: int, d_out: int, stride_elems: Optional[int] = None):
        """zl_poseidon_hash_assignments_dev: count x arity inputs at the device address d_in -> row i at d_out + i * stride_elems elements (default: the row
        length, poseidon_hash_assignment_elems(arity)); finished on return"""
        stride = self.L.zl_poseidon_hash_assignment_elems(arity) if stride_elems is None else stride_elems
        self._check(self.L.zl_poseidon_hash_assignments_dev(self._ctx, curve, arity, C.c_void_p(d_in), count, C.c_void_p(d_out), stride), "zl_poseidon_hash_assignments_dev")

    def poseidon_merkle_leaf_assignments(self, curve: int, preimages, indices, paths, depth: int) -> np.ndarray:
        """zl_poseidon_merkle_leaf_assignments: preimages (count, arity, 4), indices (count,), paths (count, depth, 4) -> (count, 2 + arity + 3 S(arity) +
        238 depth, 4), row i the complete assignment of Circuit.merkle_leaf(curve, depth, preimages[i], indices[i], paths[i])"""
        return _poseidon_merkle_leaf_assignments(self.L, self._ctx, curve, preimages, indices, paths, depth)

    def poseidon_merkle_leaf_assignments_dev(self, curve: int, arity: int, d_preimages: int, indices, d_paths: int, depth: int, d_out: int,
                                             stride_elems: Optional[int] = None):
        """zl_poseidon_merkle_leaf_assignments_dev: preimages (count x arity) and paths (count x depth) at device addresses, indices in host memory -> row i at
        d_out + i * stride_elems elements (default: the row length)"""
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        stride = self.L.zl_poseidon_merkle_leaf_assignment_elems(arity, depth) if stride_elems is None else stride_elems
        self._check(self.L.zl_poseidon_merkle_leaf_assignments_dev(self._ctx, curve, arity, C.c_void_p(d_preimages), _ptr_or_none(idx), C.c_void_p(d_paths), depth,
                                                                   idx.size, C.c_void_p(d_out), stride), "zl_poseidon_merkle_leaf_assignments_dev")

    def poseidon_merkle_leaf_member_assignments_dev(self, curve: int, arity: int, d_nodes: int, d_preimages: int, n: int, depth: int, indices, d_out: int,
                                                    stride_elems: Optional[int] = None):
        """zl_poseidon_merkle_leaf_member_assignments_dev: the memberships of the leaves `indices` (host memory) of the tree at the device address d_nodes, whose
        leaf i is the arity-`arity` hash of the preimage at element i * arity of d_preimages -> rows as poseidon_merkle_leaf_assignments_dev; a preimage that
        does not hash to its leaf is refused"""
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        stride = self.L.zl_poseidon_merkle_leaf_assignment_elems(arity, depth) if stride_elems is None else stride_elems
        self._check(self.L.zl_poseidon_merkle_leaf_member_assignments_dev(self._ctx, curve, arity, C.c_void_p(d_nodes), C.c_void_p(d_preimages), n, depth,
                                                                          _ptr_or_none(idx), idx.size, C.c_void_p(d_out), stride),
                    "zl_poseidon_merkle_leaf_member_assignments_dev")

    # ---- Groth16 ----------------------------------------------------------------------------------------------
    def groth16_prove(self, curve: int, pk: dict, r1cs: dict, assignment: np.ndarray, r: np.ndarray, s: np.ndarray):
        """pk: {'a_query','b_g1_query','h_query','l_query','b_g2_query': handles, 'alpha_g1','beta_g1','delta_g1','beta_g2',
        'delta_g2': uint64 arrays}; r1cs: {'n_constraints','n_instance','n_witness', 'A'/'B'/'C': (ptr u32, col u32, val (nnz,4) u64)}.
        Returns (a, a_inf, b, b_inf, c, c_inf) as canonical affine limb arrays."""
        cs, keep = _r1cs_struct(r1cs)
        pkc, keep_pk = _pk_struct(curve, pk)
        proof = G16ProofC()
        z = np.ascontiguousarray(assignment, dtype=np.uint64)
        self._check(self.L.zl_groth16_prove(self._ctx, C.byref(pkc), C.byref(cs), _p64(z), _p64(np.ascontiguousarray(r)),
                                            _p64(np.ascontiguousarray(s)), C.byref(proof)), "zl_groth16_prove")
        return _proof_tuple(curve, proof)

    def r1cs_upload(self, curve: int, r1cs: dict) -> int:
        """zl_r1cs_upload: the constraint matrices (r1cs as for groth16_prove) resident on this ctx's device; returns the handle"""
        cs, keep = _r1cs_struct(r1cs)
        h = C.c_uint64()
        self._check(self.L.zl_r1cs_upload(self._ctx, curve, C.byref(cs), C.byref(h)), "zl_r1cs_upload")
        return h.value

    def r1cs_free(self, handle: int):
        self._check(self.L.zl_r1cs_free(self._ctx, handle), "zl_r1cs_free")

    def groth16_prove_resident(self, curve: int, pk: dict, r1cs_handle: int, assignment: np.ndarray, r: np.ndarray, s: np.ndarray, flags: int = 0):
        """zl_groth16_prove_resident over matrices from r1cs_upload; flags: ZL_MONT = the assignment is in Montgomery form.  Returns what groth16_prove does."""
        pkc, keep_pk = _pk_struct(curve, pk)
        proof = G16ProofC()
        z = np.ascontiguousarray(assignment, dtype=np.uint64)
        self._check(self.L.zl_groth16_prove_resident(self._ctx, C.byref(pkc), r1cs_handle, _p64(z), flags, _p64(np.ascontiguousarray(r)),
                                                     _p64(np.ascontiguousarray(s)), C.byref(proof)), "zl_groth16_prove_resident")
        return _proof_tuple(curve, proof)

    def _prove_batch(self, pkc, curve: int, r1cs_handle: int, assignments: np.ndarray, r: np.ndarray, s: np.ndarray, flags: int):
        z = np.ascontiguousarray(assignments, dtype=np.uint64)
        count = z.shape[0]
        r, s = np.ascontiguousarray(r, dtype=np.uint64).reshape(count, 4), np.ascontiguousarray(s, dtype=np.uint64).reshape(count, 4)
        out = (G16ProofC * max(1, count))()
        self._check(self.L.zl_groth16_prove_batch(self._ctx, C.byref(pkc), r1cs_handle, _p64(z) if count else None, flags, _p64(r) if count else None,
                                                  _p64(s) if count else None, count, out), "zl_groth16_prove_batch")
        return [_proof_tuple(curve, p) for p in out[:count]]

    def groth16_prove_batch(self, curve: int, pk: dict, r1cs_handle: int, assignments: np.ndarray, r: np.ndarray, s: np.ndarray, flags: int = 0):
        """zl_groth16_prove_batch: assignments (count, n_variables, 4), r and s (count, 4) -> `count` proofs, proof j what groth16_prove_resident returns for
        (assignments[j], r[j], s[j]); flags as there."""
        pkc, keep_pk = _pk_struct(curve, pk)
        return self._prove_batch(pkc, curve, r1cs_handle, assignments, r, s, flags)

    def _prove_batch_dev(self, pkc, curve: int, r1cs_handle: int, d_assignments: int, count: int, r: np.ndarray, s: np.ndarray, flags: int):
        r, s = np.ascontiguousarray(r, dtype=np.uint64).reshape(count, 4), np.ascontiguousarray(s, dtype=np.uint64).reshape(count, 4)
        out = (G16ProofC * max(1, count))()
        self._check(self.L.zl_groth16_prove_batch_dev(self._ctx, C.byref(pkc), r1cs_handle, C.c_void_p(d_assignments) if count else None, flags,
                                                      _p64(r) if count else None, _p64(s) if count else None, count, out), "zl_groth16_prove_batch_dev")
        return [_proof_tuple(curve, p) for p in out[:count]]

    def groth16_prove_batch_dev(self, curve: int, pk: dict, r1cs_handle: int, d_assignments: int, count: int, r: np.ndarray, s: np.ndarray, flags: int = 0):
        """zl_groth16_prove_batch_dev: groth16_prove_batch over `count` dense assignments at the device address d_assignments"""
        pkc, keep_pk = _pk_struct(curve, pk)
        return self._prove_batch_dev(pkc, curve, r1cs_handle, d_assignments, count, r, s, flags)

    def _prove_chains(self, pkc, curve: int, r1cs_handle: int, k: int, x0, x1, r: np.ndarray, s: np.ndarray):
        a, b = _elems(x0, 1), _elems(x1, 1)
        count = a.shape[0]
        assert b.shape == a.shape
        r, s = np.ascontiguousarray(r, dtype=np.uint64).reshape(count, 4), np.ascontiguousarray(s, dtype=np.uint64).reshape(count, 4)
        out = (G16ProofC * max(1, count))()
        pub = np.zeros((count, 4), dtype=np.uint64)
        self._check(self.L.zl_groth16_prove_poseidon_chains(self._ctx, C.byref(pkc), r1cs_handle, k, _ptr_or_none(a), _ptr_or_none(b), _ptr_or_none(r), _ptr_or_none(s),
                                                            count, out, _ptr_or_none(pub)), "zl_groth16_prove_poseidon_chains")
        return [_proof_tuple(curve, p) for p in out[:count]], pub

    def groth16_prove_poseidon_chains(self, curve: int, pk: dict, r1cs_handle: int, k: int, x0, x1, r: np.ndarray, s: np.ndarray):
        """zl_groth16_prove_poseidon_chains: chain inputs x0, x1 (count, 4) and blinding scalars -> (`count` proofs, the public inputs h_k (count, 4)); the
        assignments are made on the device and never leave it"""
        pkc, keep_pk = _pk_struct(curve, pk)
        return self._prove_chains(pkc, curve, r1cs_handle, k, x0, x1, r, s)

    def _prove_merkle_paths(self, pkc, curve: int, r1cs_handle: int, depth: int, leaves, indices, paths, r: np.ndarray, s: np.ndarray):
        lv = _elems(leaves, 1)
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        pa = np.ascontiguousarray(np.asarray(paths, dtype=np.uint64).reshape(-1, max(1, depth), 4))
        count = idx.size
        assert lv.shape[0] == count and pa.shape[0] == count
        r, s = np.ascontiguousarray(r, dtype=np.uint64).reshape(count, 4), np.ascontiguousarray(s, dtype=np.uint64).reshape(count, 4)
        out = (G16ProofC * max(1, count))()
        roots = np.zeros((count, 4), dtype=np.uint64)
        self._check(self.L.zl_groth16_prove_merkle_paths(self._ctx, C.byref(pkc), r1cs_handle, depth, _ptr_or_none(lv), _ptr_or_none(idx), _ptr_or_none(pa),
                                                         _ptr_or_none(r), _ptr_or_none(s), count, out, _ptr_or_none(roots)), "zl_groth16_prove_merkle_paths")
        return [_proof_tuple(curve, p) for p in out[:count]], roots

    def groth16_prove_merkle_paths(self, curve: int, pk: dict, r1cs_handle: int, depth: int, leaves, indices, paths, r: np.ndarray, s: np.ndarray):
        """zl_groth16_prove_merkle_paths: leaves (count, 4), indices (count,), paths (count, depth, 4) and blinding scalars -> (`count` proofs, the roots
        (count, 4): each proof's public input); the assignments are made on the device and never leave it"""
        pkc, keep_pk = _pk_struct(curve, pk)
        return self._prove_merkle_paths(pkc, curve, r1cs_handle, depth, leaves, indices, paths, r, s)

    def _prove_merkle_members(self, pkc, curve: int, r1cs_handle: int, d_nodes: int, n: int, depth: int, indices, r: np.ndarray, s: np.ndarray):
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        count = idx.size
        r, s = np.ascontiguousarray(r, dtype=np.uint64).reshape(count, 4), np.ascontiguousarray(s, dtype=np.uint64).reshape(count, 4)
        out = (G16ProofC * max(1, count))()
        root = np.zeros(4, dtype=np.uint64)
        self._check(self.L.zl_groth16_prove_merkle_members(self._ctx, C.byref(pkc), r1cs_handle, C.c_void_p(d_nodes), n, depth, _ptr_or_none(idx), _ptr_or_none(r),
                                                           _ptr_or_none(s), count, out, _p64(root)), "zl_groth16_prove_merkle_members")
        return [_proof_tuple(curve, p) for p in out[:count]], root

    def groth16_prove_merkle_members(self, curve: int, pk: dict, r1cs_handle: int, d_nodes: int, n: int, depth: int, indices, r: np.ndarray, s: np.ndarray):
        """zl_groth16_prove_merkle_members: the tree at the device address d_nodes (n leaves, `depth` levels), leaf indices (count,) and blinding scalars ->
        (`count` proofs of membership, the tree's root (4,): every proof's public input; zero when count == 0)"""
        pkc, keep_pk = _pk_struct(curve, pk)
        return self._prove_merkle_members(pkc, curve, r1cs_handle, d_nodes, n, depth, indices, r, s)

    def _prove_hashes(self, pkc, curve: int, r1cs_handle: int, arity: int, inputs, r: np.ndarray, s: np.ndarray):
        v = _elems(inputs, max(1, arity))
        count = v.shape[0]
        r, s = np.ascontiguousarray(r, dtype=np.uint64).reshape(count, 4), np.ascontiguousarray(s, dtype=np.uint64).reshape(count, 4)
        out = (G16ProofC * max(1, count))()
        pub = np.zeros((count, 4), dtype=np.uint64)
        self._check(self.L.zl_groth16_prove_poseidon_hashes(self._ctx, C.byref(pkc), r1cs_handle, arity, _ptr_or_none(v), _ptr_or_none(r), _ptr_or_none(s), count, out,
                                                            _ptr_or_none(pub)), "zl_groth16_prove_poseidon_hashes")
        return [_proof_tuple(curve, p) for p in out[:count]], pub

    def _prove_encryptions(self, pkc, curve: int, r1cs_handle: int, initial_state, keys, headers, plaintexts, r: np.ndarray, s: np.ndarray):
        k, h, t = _duplex_operands(keys, headers, plaintexts)
        count, blocks, width = t.shape[0], t.shape[1], t.shape[2] + 1
        st = _duplex_state(initial_state, width)
        r, s = np.ascontiguousarray(r, dtype=np.uint64).reshape(count, 4), np.ascontiguousarray(s, dtype=np.uint64).reshape(count, 4)
        out = (G16ProofC * max(1, count))()
        tags, cts = np.zeros((count, 4), dtype=np.uint64), np.zeros_like(t)
        self._check(self.L.zl_groth16_prove_poseidon_encryptions(self._ctx, C.byref(pkc), r1cs_handle, width, None if st is None else _p64(st), _ptr_or_none(k), k.shape[1],
                                                                 _ptr_or_none(h), h.shape[1], _ptr_or_none(t), blocks, _ptr_or_none(r), _ptr_or_none(s), count, out,
                                                                 _ptr_or_none(tags), _ptr_or_none(cts)), "zl_groth16_prove_poseidon_encryptions")
        return [_proof_tuple(curve, p) for p in out[:count]], tags, cts

    def groth16_prove_poseidon_encryptions(self, curve: int, pk: dict, r1cs_handle: int, initial_state, keys, headers, plaintexts, r: np.ndarray, s: np.ndarray):
        """zl_groth16_prove_poseidon_encryptions: operands as poseidon_duplex_encrypt and blinding scalars -> (`count` proofs, tags (count, 4), ciphertexts (count,
        N, W - 1, 4)): the public inputs of proof j are tags[j], ciphertexts[j] and headers[j]"""
        pkc, keep_pk = _pk_struct(curve, pk)
        return self._prove_encryptions(pkc, curve, r1cs_handle, initial_state, keys, headers, plaintexts, r, s)

    def groth16_prove_poseidon_hashes(self, curve: int, pk: dict, r1cs_handle: int, arity: int, inputs, r: np.ndarray, s: np.ndarray):
        """zl_groth16_prove_poseidon_hashes: inputs (count, arity, 4) and blinding scalars -> (`count` proofs, the digests (count, 4): each proof's public input)"""
        pkc, keep_pk = _pk_struct(curve, pk)
        return self._prove_hashes(pkc, curve, r1cs_handle, arity, inputs, r, s)

    def _prove_merkle_leaf_paths(self, pkc, curve: int, r1cs_handle: int, arity: int, depth: int, preimages, indices, paths, r: np.ndarray, s: np.ndarray):
        pre = _elems(preimages, max(1, arity))
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        pa = np.ascontiguousarray(np.asarray(paths, dtype=np.uint64).reshape(-1, max(1, depth), 4))
        count = idx.size
        assert pre.shape[0] == count and pa.shape[0] == count
        r, s = np.ascontiguousarray(r, dtype=np.uint64).reshape(count, 4), np.ascontiguousarray(s, dtype=np.uint64).reshape(count, 4)
        out = (G16ProofC * max(1, count))()
        roots = np.zeros((count, 4), dtype=np.uint64)
        self._check(self.L.zl_groth16_prove_merkle_leaf_paths(self._ctx, C.byref(pkc), r1cs_handle, arity, depth, _ptr_or_none(pre), _ptr_or_none(idx), _ptr_or_none(pa),
                                                              _ptr_or_none(r), _ptr_or_none(s), count, out, _ptr_or_none(roots)), "zl_groth16_prove_merkle_leaf_paths")
        return [_proof_tuple(curve, p) for p in out[:count]], roots

    def groth16_prove_merkle_leaf_paths(self, curve: int, pk: dict, r1cs_handle: int, arity: int, depth: int, preimages, indices, paths, r: np.ndarray, s: np.ndarray):
        """zl_groth16_prove_merkle_leaf_paths: preimages (count, arity, 4), indices (count,), paths (count, depth, 4) and blinding scalars -> (`count` proofs, the
        roots (count, 4): each proof's public input)"""
        pkc, keep_pk = _pk_struct(curve, pk)
        return self._prove_merkle_leaf_paths(pkc, curve, r1cs_handle, arity, depth, preimages, indices, paths, r, s)

    def _prove_merkle_leaf_members(self, pkc, curve: int, r1cs_handle: int, arity: int, d_nodes: int, d_preimages: int, n: int, depth: int, indices, r: np.ndarray,
                                   s: np.ndarray):
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        count = idx.size
        r, s = np.ascontiguousarray(r, dtype=np.uint64).reshape(count, 4), np.ascontiguousarray(s, dtype=np.uint64).reshape(count, 4)
        out = (G16ProofC * max(1, count))()
        root = np.zeros(4, dtype=np.uint64)
        self._check(self.L.zl_groth16_prove_merkle_leaf_members(self._ctx, C.byref(pkc), r1cs_handle, arity, C.c_void_p(d_nodes), C.c_void_p(d_preimages), n, depth,
                                                                _ptr_or_none(idx), _ptr_or_none(r), _ptr_or_none(s), count, out, _p64(root)),
                    "zl_groth16_prove_merkle_leaf_members")
        return [_proof_tuple(curve, p) for p in out[:count]], root

    def groth16_prove_merkle_leaf_members(self, curve: int, pk: dict, r1cs_handle: int, arity: int, d_nodes: int, d_preimages: int, n: int, depth: int, indices,
                                          r: np.ndarray, s: np.ndarray):
        """zl_groth16_prove_merkle_leaf_members: the tree at the device address d_nodes (n leaves, `depth` levels), the n x arity preimages of its leaves at
        d_preimages, leaf indices (count,) and blinding scalars -> (`count` proofs, the tree's root (4,))"""
        pkc, keep_pk = _pk_struct(curve, pk)
        return self._prove_merkle_leaf_members(pkc, curve, r1cs_handle, arity, d_nodes, d_preimages, n, depth, indices, r, s)

    def _prove_forest_members(self, pkc, curve: int, r1cs_handle: int, forest: "MerkleForest", tree_of, indices, r: np.ndarray, s: np.ndarray):
        tr, idx = _forest_items(tree_of, indices)
        count = idx.size
        r, s = np.ascontiguousarray(r, dtype=np.uint64).reshape(count, 4), np.ascontiguousarray(s, dtype=np.uint64).reshape(count, 4)
        out = (G16ProofC * max(1, count))()
        roots = np.zeros((count, 4), dtype=np.uint64)
        self._check(self.L.zl_groth16_prove_forest_members(self._ctx, C.byref(pkc), r1cs_handle, forest._f, _p32(tr), _ptr_or_none(idx), _ptr_or_none(r), _ptr_or_none(s),
                                                           count, out, _ptr_or_none(roots)), "zl_groth16_prove_forest_members")
        return [_proof_tuple(curve, p) for p in out[:count]], roots

    def groth16_last_h(self, n: int) -> np.ndarray:
        out = np.zeros((n, 4), dtype=np.uint64)
        self._check(self.L.zl_groth16_last_h(self._ctx, _p64(out), n), "zl_groth16_last_h")
        return out


class ShardedGroth16Keys:
    """a proving key spread over the ranks of a MultiBackend (zl_g16_shard per rank) + the constraint matrices on rank 0"""

    def __init__(self, mb: "MultiBackend", curve: int, pk: dict, r1cs: dict, cuts=None):
        self.mb, self.curve, self.L = mb, curve, mb.L
        G = mb.size
        ni, nw = r1cs["n_instance"], r1cs["n_witness"]
        nv = ni + nw
        n_h = pk["h_query"].shape[0]

        def bounds(total):
            if cuts is not None:
                edges = [0] + [int(round(total * f)) for f in cuts] + [total]
            else:
                edges = [total * g // G for g in range(G + 1)]
            return [(edges[g], max(0, edges[g + 1] - edges[g])) for g in range(G)]

        vb, wb, hb = bounds(nv), bounds(nw), bounds(n_h)
        self.shards = (G16ShardC * G)()
        self._made, self._keep, self._r1cs = [], [], 0
        try:
            for g in range(G):
                be = mb.ranks[g]
                sh = self.shards[g]
                (sh.var_first, sh.var_count), (sh.wit_first, sh.wit_count), (sh.h_first, sh.h_count) = vb[g], wb[g], hb[g]
                for name, (f, c), grp in (("a_query", vb[g], ZL_G1), ("b_g1_query", vb[g], ZL_G1), ("h_query", hb[g], ZL_G1), ("l_query", wb[g], ZL_G1),
                                          ("b_g2_query", vb[g], ZL_G2)):
                    if c == 0:
                        continue
                    hnd = be.bases_upload(curve, np.ascontiguousarray(pk[name][f:f + c]), group=grp)
                    self._made.append((be, hnd))
                    setattr(sh, name, hnd)
            cs = R1csC()
            cs.n_constraints, cs.n_instance, cs.n_witness = r1cs["n_constraints"], ni, nw
            keep = []
            for m, key in enumerate("ABC"):
                ptr, col, val = (np.ascontiguousarray(x, dtype=t) for x, t in zip(r1cs[key], (np.uint32, np.uint32, np.uint64)))
                keep += [ptr, col, val]
                cs.row_ptr[m] = ptr.ctypes.data_as(C.POINTER(C.c_uint32))
                cs.col[m] = col.ctypes.data_as(C.POINTER(C.c_uint32))
                cs.val[m] = val.ctypes.data_as(u64p)
            hr = C.c_uint64()
            be0 = mb.ranks[0]
            be0._check(self.L.zl_r1cs_upload(be0._ctx, curve, C.byref(cs), C.byref(hr)), "zl_r1cs_upload")
            self._r1cs = hr.value
            self.pkc = G16PkC()
            self.pkc.curve = curve
            for k in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2"):
                arr = np.ascontiguousarray(pk[k], dtype=np.uint64)
                self._keep.append(arr)
                setattr(self.pkc, k, arr.ctypes.data_as(u64p))
        except Exception:
            self.close()
            raise

    def rank_handles(self, g: int) -> dict:
        """rank g's shard: {query name: (handle on ranks[g], points in it)} for the queries it holds a slice of (e.g. for ranks[g].bases_precompute)"""
        sh = self.shards[g]
        counts = {"a_query": sh.var_count, "b_g1_query": sh.var_count, "h_query": sh.h_count, "l_query": sh.wit_count, "b_g2_query": sh.var_count}
        return {name: (int(getattr(sh, name)), int(n)) for name, n in counts.items() if n}

    def prove(self, assignment: np.ndarray, r: np.ndarray, s: np.ndarray, mont: bool = False):
        proof = G16ProofC()
        z = np.ascontiguousarray(assignment, dtype=np.uint64)
        rc = self.L.zl_groth16_prove_sharded(self.mb._m, C.byref(self.pkc), self.shards, self._r1cs, _p64(z), ZL_MONT if mont else 0, _p64(np.ascontiguousarray(r)),
                                             _p64(np.ascontiguousarray(s)), C.byref(proof))
        if rc:
            raise BackendError(rc, "zl_groth16_prove_sharded", self.L.zl_strerror(rc).decode())
        nq = FQ_LIMBS[self.curve]
        return (np.array(proof.a[: 2 * nq], dtype=np.uint64), proof.a_inf, np.array(proof.b[: 4 * nq], dtype=np.uint64), proof.b_inf,
                np.array(proof.c[: 2 * nq], dtype=np.uint64), proof.c_inf)

    def close(self):
        for be, hnd in self._made:
            try:
                be.bases_free(hnd)
            except Exception:
                pass
        self._made = []
        if self._r1cs:
            self.L.zl_r1cs_free(self.mb.ranks[0]._ctx, self._r1cs)
            self._r1cs = 0


class MultiBackend:
    """zl_mctx: G devices driven from one process (include/zl_backend.h, multi-GPU section).  ranks[g] is a Backend bound to rank g's
    ctx (upload / generate that rank's shard of the bases there); device ids may repeat (virtual ranks on one GPU, test mode)."""

    def __init__(self, device_ids):
        self.L = load_library()
        self._m = C.c_void_p()
        ids = (C.c_int * len(device_ids))(*device_ids)
        rc = self.L.zl_ctx_create_multi(C.byref(self._m), ids, len(device_ids))
        if rc:
            raise BackendError(rc, "zl_ctx_create_multi", self.L.zl_strerror(rc).decode())
        self.size = self.L.zl_mctx_size(self._m)
        self.ranks = [Backend(_borrowed_ctx=self.L.zl_mctx_ctx(self._m, g)) for g in range(self.size)]
        self.uses_rccl = bool(self.L.zl_mctx_uses_rccl(self._m))

    def msm_sharded(self, handles, d_scalars, counts, firsts=None) -> Tuple[np.ndarray, int]:
        """handles[g]: bases handle on rank g; d_scalars[g]: device pointer (on rank g's device) to counts[g] x 4 u64 canonical scalars"""
        G = self.size
        curve, group, _ = self.ranks[0]._bases[handles[0]]
        hs = np.array(handles, dtype=np.uint64)
        ptrs = (C.c_void_p * G)(*[int(p) for p in d_scalars])
        ns = (C.c_size_t * G)(*[int(c) for c in counts])
        fs = (C.c_size_t * G)(*[int(f) for f in (firsts or [0] * G)])
        out, inf = np.zeros(2 * group * FQ_LIMBS[curve], dtype=np.uint64), C.c_uint8(0)
        rc = self.L.zl_msm_sharded(self._m, _p64(hs), fs, ptrs, ns, _p64(out), C.byref(inf))
        if rc:
            raise BackendError(rc, "zl_msm_sharded", self.L.zl_strerror(rc).decode())
        return out, inf.value

    def groth16_shard_keys(self, curve: int, pk: dict, r1cs: dict, cuts=None) -> "ShardedGroth16Keys":
        """Spread a proving key over the ranks of this mctx for zl_groth16_prove_sharded.  pk: the key as HOST arrays of canonical affine points ('a_query' ... as
        (n, words) uint64, all-zero row = infinity) + the five single points; every query is cut into contiguous slices (cuts: optional fractions at which to
        cut, default equal parts), rank g uploads its slices to its own ctx, rank 0 uploads the matrices."""
        return ShardedGroth16Keys(self, curve, pk, r1cs, cuts)

    def groth16_prove_sharded(self, curve: int, pk: dict, r1cs: dict, assignment: np.ndarray, r: np.ndarray, s: np.ndarray, cuts=None):
        """upload + one proof + free (tests); returns (a, a_inf, b, b_inf, c, c_inf)"""
        keys = self.groth16_shard_keys(curve, pk, r1cs, cuts)
        try:
            return keys.prove(assignment, r, s)
        finally:
            keys.close()

    def ntt_sharded(self, curve: int, d_data, log_n: int, inverse: bool = False, coset: bool = False, mont: bool = False):
        G = self.size
        ptrs = (C.c_void_p * G)(*[int(p) for p in d_data])
        flags = (ZL_INVERSE if inverse else 0) | (ZL_COSET if coset else 0) | (ZL_MONT if mont else 0)
        rc = self.L.zl_ntt_sharded(self._m, curve, ptrs, log_n, flags)
        if rc:
            raise BackendError(rc, "zl_ntt_sharded", self.L.zl_strerror(rc).decode())

    def close(self):
        if self._m:
            for r in self.ranks:
                r.close()
            self.L.zl_mctx_destroy(self._m)
            self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- test-only hooks (include/zl_backend_test.h): device Poseidon KAT, raw-limb field / point access ---------------------------------
TEST_ABI_SYMBOLS = ["zl_test_poseidon_permute_dev", "zl_test_fp28_op", "zl_test_fp28_bn_op", "zl_test_pairing_product", "zl_test_point_op", "zl_test_circuit_tweak", "zl_test_fq_mul_rate", "zl_test_fr28_op", "zl_test_fr29_op",
                    "zl_test_poseidon_permute_dev28r", "zl_test_fq_mul_clock", "zl_test_acc_clock", "zl_test_acc_clock_read", "zl_test_clock_probe_launch", "zl_test_clock_probe_read",
                    "zl_test_miller_dev", "zl_test_final_exp", "zl_test_verify_batch_host", "zl_test_ntt_plan", "zl_test_ntt_fit_beside", "zl_test_fp2pair_op", "zl_test_point_form_op",
                    "zl_test_endo_split", "zl_test_endo_split_inf", "zl_test_decode_points_host", "zl_test_fq2_sqrt",
                    "zl_test_final_exp_dev", "zl_test_fq12_inverse", "zl_test_fq12_zeta", "zl_test_pairing_product_scaled",
                    "zl_test_msm_plan", "zl_test_msm_batch_form", "zl_test_msm_exact_cover", "zl_test_fp_op"]


def _p32(a: np.ndarray):
    assert a.dtype == np.uint32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def groth16_keys_parse(curve: int, data: bytes, check: bool = False) -> int:
    """host-only validation of ProvingContext bytes (zl_groth16_keys_parse): the C error code (0 = acceptable framing)"""
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data if data else b"\0")
    return int(load_library().zl_groth16_keys_parse(curve, buf, len(data), ZL_CHECK if check else 0))


def hook_ntt_plan(log_n: int) -> list[int]:
    """the pass sizes zl_ntt.hip's driver uses for a 2^log_n-point transform (zl_test_ntt_plan; host only)"""
    P = C.c_uint(0)
    sizes = (C.c_uint * 4)()
    rc = load_library().zl_test_ntt_plan(log_n, C.byref(P), sizes)
    if rc != 0:
        raise BackendError(rc, "zl_test_ntt_plan")
    assert all(sizes[k] == 0 for k in range(P.value, 4))
    return [int(sizes[k]) for k in range(P.value)]


def hook_ntt_fit_beside(be: "Backend", on: bool) -> bool:
    """set the ctx's ntt_fit_beside (the 96-register instantiations of the NTT passes); returns the previous setting"""
    old = be.L.zl_test_ntt_fit_beside(be._ctx, int(on))
    if old < 0:
        raise BackendError(old, "zl_test_ntt_fit_beside")
    return bool(old)


def hook_msm_exact_cover(be: "Backend", mode: int) -> int:
    """force (1), forbid (-1) or leave to the planner (0) the exact-cover plan of BLS12-381 G1 MSMs on this ctx (zl_test_msm_exact_cover); returns the previous mode"""
    old = C.c_int(0)
    be.L.zl_test_msm_exact_cover.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    be._check(be.L.zl_test_msm_exact_cover(be._ctx, int(mode), C.byref(old)), "zl_test_msm_exact_cover")
    return int(old.value)


def hook_endo_split(be: "Backend", curve: int, group: int, scalars: np.ndarray, inf: Optional[np.ndarray] = None):
    """the scalar split in front of the group's plain MSM, alone (zl_test_endo_split / _inf): scalars (n, 4) uint64, inf (n,) uint8 flags of bases at infinity or
    None -> (records (endo_k, n, 8) uint32: magnitude in the low words, sign in bit 31 of word 7; the kernel's bad flags; endo_k; bits per part)"""
    s = np.ascontiguousarray(scalars, dtype=np.uint64)
    n = s.shape[0]
    assert s.shape == (n, 4)
    out = np.zeros(4 * n * 8 + 1, dtype=np.uint32)
    k, bits = C.c_int(0), C.c_int(0)
    # declared here, not in load_library: the loader then also takes a build from before the hook (the parent side of tools/ab/bn254_g2_gls_ab.sh)
    tail = [C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    be.L.zl_test_endo_split.argtypes = [C.c_void_p, C.c_int, C.c_int, u64p] + tail
    be.L.zl_test_endo_split_inf.argtypes = [C.c_void_p, C.c_int, C.c_int, u64p, u8p] + tail
    if inf is None:
        rc = be.L.zl_test_endo_split(be._ctx, curve, group, _p64(s), n, _p32(out), C.byref(k), C.byref(bits))
    else:
        f = np.ascontiguousarray(inf, dtype=np.uint8)
        assert f.shape == (n,)
        rc = be.L.zl_test_endo_split_inf(be._ctx, curve, group, _p64(s), f.ctypes.data_as(u8p), n, _p32(out), C.byref(k), C.byref(bits))
    be._check(rc, "zl_test_endo_split")
    return out[: k.value * n * 8].reshape(k.value, n, 8).copy(), int(out[k.value * n * 8]), k.value, bits.value


class MsmPlanC(C.Structure):
    """zl_test_msm_plan_t (include/zl_backend_test.h)"""
    _fields_ = [(f, C.c_int32) for f in ("c W SETS NB sc_bits glv endo_k wide pre chunk nchunks big_span red_g0 red_levels spread_t nslices per_slice fsl Gn "
                                         "sort_lds lds_prefix_small lds_ranges fine_cap fine_threads acc_quad tail_quad_max by_cuts may_big may_giant").split()]

    def __repr__(self):
        return "MsmPlan(" + ", ".join(f"{f}={getattr(self, f)}" for f, _ in self._fields_) + ")"


def hook_msm_plan(be: "Backend", handle: int, n: int, first: int = 0) -> MsmPlanC:
    """the plan of the next single MSM over points [first, first + n) of the handle, under the ctx's forced window and the ZL_TUNE_* environment of the moment
    (zl_test_msm_plan: MsmJob::plan alone, nothing launched or allocated), with the launch forms the driver derives from it"""
    p = MsmPlanC()
    be.L.zl_test_msm_plan.argtypes = [C.c_void_p, C.c_uint64, C.c_size_t, C.c_size_t, C.POINTER(MsmPlanC)]
    be._check(be.L.zl_test_msm_plan(be._ctx, handle, first, n, C.byref(p)), "zl_test_msm_plan")
    return p


def hook_msm_batch_form(count: int, biggest: int) -> dict:
    """how the job driver runs a batch of `count` MSMs, the biggest of `biggest` points (zl_test_msm_batch_form; host only): side (side-by-side lanes, else the
    three-stream pipeline), lanes (buffer sets in rotation), phased (phase-major issue)"""
    L = load_library()
    L.zl_test_msm_batch_form.argtypes = [C.c_size_t, C.c_uint64, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    s, l, p = C.c_int(0), C.c_int(0), C.c_int(0)
    rc = L.zl_test_msm_batch_form(count, biggest, C.byref(s), C.byref(l), C.byref(p))
    if rc != 0:
        raise BackendError(rc, "zl_test_msm_batch_form")
    return {"side": bool(s.value), "lanes": l.value, "phased": bool(p.value)}


def hook_poseidon_permute_dev(be: "Backend", curve: int, state: np.ndarray) -> np.ndarray:
    """width-3 Poseidon permutation computed on the device with the device Fr arithmetic (canonical (3,4) uint64 in / out)"""
    st = np.ascontiguousarray(state.copy(), dtype=np.uint64)
    be._check(be.L.zl_test_poseidon_permute_dev(be._ctx, curve, _p64(st)), "zl_test_poseidon_permute_dev")
    return st


def hook_poseidon_permute_dev28r(be: "Backend", curve: int, state: np.ndarray) -> np.ndarray:
    """the same permutation through the lazily reduced 10 x 28-bit Fr multiplier of the NTT passes (zl_field28r.h)"""
    st = np.ascontiguousarray(state.copy(), dtype=np.uint64)
    be._check(be.L.zl_test_poseidon_permute_dev28r(be._ctx, curve, _p64(st)), "zl_test_poseidon_permute_dev28r")
    return st


def hook_fp28_op(be: Optional["Backend"], op: int, operands: np.ndarray, bn254: bool = False) -> np.ndarray:
    """operands: (n, 4, L) uint32 raw limbs -> (n, L), L = 14 (BLS12-381 Fq) or 10 (bn254=True: BN254 Fq); be = None runs the host code path"""
    a = np.ascontiguousarray(operands, dtype=np.uint32)
    n, limbs = a.shape[0], (10 if bn254 else 14)
    assert a.shape[1:] == (4, limbs)
    out = np.zeros((n, limbs), dtype=np.uint32)
    L = load_library()
    fn = L.zl_test_fp28_bn_op if bn254 else L.zl_test_fp28_op
    rc = fn(be._ctx if be is not None else None, op, _p32(a), n, _p32(out))
    if rc:
        raise BackendError(rc, "zl_test_fp28_bn_op" if bn254 else "zl_test_fp28_op")
    return out


def hook_pairing_product(curve: int, ps: np.ndarray, qs: np.ndarray) -> np.ndarray:
    """prod_i e(P_i, Q_i) through the lock-step Miller loops (host only): ps (n, 2 FQ64) / qs (n, 4 FQ64) canonical u64 words -> 12 x FQ64 words"""
    p = np.ascontiguousarray(ps, dtype=np.uint64)
    q = np.ascontiguousarray(qs, dtype=np.uint64)
    n = p.shape[0]
    out = np.zeros((12, p.shape[1] // 2), dtype=np.uint64)
    rc = load_library().zl_test_pairing_product(curve, n, _p64(p), _p64(q), _p64(out))
    if rc:
        raise BackendError(rc, "zl_test_pairing_product")
    return out


def hook_miller_dev(be: "Backend", curve: int, ps: np.ndarray, qs: np.ndarray) -> np.ndarray:
    """the raw device Miller value of every pair (zl_test_miller_dev): ps (n, 2 FQ64) / qs (n, 4 FQ64) -> (n, 12, FQ64) canonical words"""
    p = np.ascontiguousarray(ps, dtype=np.uint64)
    q = np.ascontiguousarray(qs, dtype=np.uint64)
    out = np.zeros((p.shape[0], 12, FQ_LIMBS[curve]), dtype=np.uint64)
    be._check(be.L.zl_test_miller_dev(be._ctx, curve, p.shape[0], _p64(p), _p64(q), _p64(out)), "zl_test_miller_dev")
    return out


def hook_pairing_product_scaled(be: "Backend", curve: int, ps: np.ndarray, qs: np.ndarray, scalars128: Optional[np.ndarray]) -> np.ndarray:
    """prod_i e(k_i P_i, Q_i) through the production Miller-product driver with its scalars (zl_test_pairing_product_scaled): ps (n, 2 FQ64) / qs (n, 4 FQ64)
    canonical words, scalars128 (n, 2) u64 little-endian or None -> 12 x FQ64 canonical words"""
    nq = FQ_LIMBS[curve]
    p = np.ascontiguousarray(np.asarray(ps, dtype=np.uint64).reshape(-1, 2 * nq))
    q = np.ascontiguousarray(np.asarray(qs, dtype=np.uint64).reshape(-1, 4 * nq))
    n = p.shape[0]
    assert q.shape[0] == n
    k = None
    if scalars128 is not None:
        k = np.ascontiguousarray(scalars128, dtype=np.uint64)
        assert k.shape == (n, 2)
    if n == 0:
        p, q = np.zeros((1, 2 * nq), dtype=np.uint64), np.zeros((1, 4 * nq), dtype=np.uint64)
    out = np.zeros((12, nq), dtype=np.uint64)
    be._check(be.L.zl_test_pairing_product_scaled(be._ctx, curve, n, _p64(p), _p64(q), _p64(k) if k is not None and n else None, _p64(out)),
              "zl_test_pairing_product_scaled")
    return out


def hook_final_exp(curve: int, f: np.ndarray) -> np.ndarray:
    """the host final exponentiation of 12 canonical coefficients (zl_test_final_exp)"""
    a = np.ascontiguousarray(f, dtype=np.uint64)
    out = np.zeros((12, FQ_LIMBS[curve]), dtype=np.uint64)
    rc = load_library().zl_test_final_exp(curve, _p64(a), _p64(out))
    if rc:
        raise BackendError(rc, "zl_test_final_exp")
    return out


def hook_final_exp_dev(be: "Backend", curve: int, f: np.ndarray):
    """the device final exponentiation (zl_test_final_exp_dev) of (count, 12, FQ64) canonical values -> (values of the same shape, singular (count,) uint8)"""
    a = np.ascontiguousarray(np.asarray(f, dtype=np.uint64).reshape(-1, 12, FQ_LIMBS[curve]))
    out = np.zeros_like(a)
    sing = np.zeros(max(1, a.shape[0]), dtype=np.uint8)
    be._check(be.L.zl_test_final_exp_dev(be._ctx, curve, a.shape[0], _p64(a if a.size else np.zeros(1, dtype=np.uint64)),
                                         _p64(out if out.size else np.zeros(1, dtype=np.uint64)), sing.ctypes.data_as(u8p)), "zl_test_final_exp_dev")
    return out, sing[:a.shape[0]]


def hook_fq12_inverse(curve: int, f: np.ndarray):
    """the inverse in Fq12 by the norm chain the device final exponentiation uses, on the host (zl_test_fq12_inverse): 12 canonical coefficients ->
    (12 canonical coefficients, singular)"""
    a = np.ascontiguousarray(np.asarray(f, dtype=np.uint64).reshape(12, FQ_LIMBS[curve]))
    out = np.zeros_like(a)
    sing = np.zeros(1, dtype=np.uint8)
    rc = load_library().zl_test_fq12_inverse(curve, _p64(a), _p64(out), sing.ctypes.data_as(u8p))
    if rc:
        raise BackendError(rc, "zl_test_fq12_inverse")
    return out, bool(sing[0])


def hook_fq12_zeta(curve: int) -> np.ndarray:
    """the cube root of unity in Fq of the inverse chain (zl_test_fq12_zeta), canonical words"""
    out = np.zeros(FQ_LIMBS[curve], dtype=np.uint64)
    rc = load_library().zl_test_fq12_zeta(curve, _p64(out))
    if rc:
        raise BackendError(rc, "zl_test_fq12_zeta")
    return out


def _proofs_array(proofs):
    arr = (G16ProofC * max(1, len(proofs)))()
    for i, pr in enumerate(proofs):
        arr[i] = _proof_struct(pr)
    return arr


def _pubs_of(public_inputs, count: int, n_public: int) -> np.ndarray:
    pub = np.ascontiguousarray(np.asarray(public_inputs, dtype=np.uint64).reshape(-1))
    assert pub.size == count * n_public * 4, "public_inputs: count x n_public x 4 words"
    return pub if pub.size else np.zeros(4, dtype=np.uint64)


def hook_verify_batch_host(curve: int, vk: dict, proofs, public_inputs, n_public: int, seed: Optional[int] = 0):
    """zl_test_verify_batch_host: the batch verifier's random linear combination on the host.  vk: alpha_g1, beta_g2, gamma_g2, delta_g2 (canonical
    words) and gamma_abc ((n_public + 1) G1 points); proofs: (a, a_inf, b, b_inf, c, c_inf) tuples.  Returns (ok, per-proof verdicts)."""
    n = len(proofs)
    arr = _proofs_array(proofs)
    pub = _pubs_of(public_inputs, n, n_public)
    vks = {k: np.ascontiguousarray(vk[k], dtype=np.uint64) for k in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc")}
    sd = np.array([seed or 0], dtype=np.uint64)
    ok = C.c_int(0)
    each = np.zeros(max(1, n), dtype=np.uint8)
    rc = load_library().zl_test_verify_batch_host(curve, _p64(vks["alpha_g1"]), _p64(vks["beta_g2"]), _p64(vks["gamma_g2"]), _p64(vks["delta_g2"]),
                                                  _p64(vks["gamma_abc"]), n_public, arr, _p64(pub), n, _p64(sd) if seed is not None else None,
                                                  C.byref(ok), each.ctypes.data_as(u8p))
    if rc:
        raise BackendError(rc, "zl_test_verify_batch_host")
    return bool(ok.value), each[:n].astype(bool)


def hook_decode_points_host(curve: int, group: int, data, count: int):
    """zl_test_decode_points_host: the device decoders' templates (csrc/zl_decode.h) run on the CPU; arguments and results as Backend.points_from_bytes"""
    L = load_library()
    buf = _bytes_view(data, 0, count * L.zl_point_bytes(curve, group))
    xy = np.zeros((max(1, count), 2 * group * FQ_LIMBS[curve]), dtype=np.uint64)
    inf = np.zeros(max(1, count), dtype=np.uint8)
    st = np.zeros(max(1, count), dtype=np.int32)
    rc = L.zl_test_decode_points_host(curve, group, _addr(buf, 0), count, _p64(xy), inf.ctypes.data_as(u8p), st.ctypes.data_as(i32p))
    if rc:
        raise BackendError(rc, "zl_test_decode_points_host")
    return xy[:count], inf[:count], st[:count]


def hook_fq2_sqrt(be: Optional["Backend"], curve: int, values: np.ndarray):
    """zl_test_fq2_sqrt: values (n, 2 FQ64) canonical words c0 || c1 -> (roots (n, 2 FQ64), all-zero where there is none; ok (n,) bool); be = None: host"""
    a = np.ascontiguousarray(values, dtype=np.uint64)
    n = a.shape[0]
    assert a.shape == (n, 2 * FQ_LIMBS[curve])
    out = np.zeros_like(a)
    ok = np.zeros(max(1, n), dtype=np.uint8)
    rc = load_library().zl_test_fq2_sqrt(be._ctx if be is not None else None, curve, _p64(a) if n else None, n, _p64(out) if n else None, ok.ctypes.data_as(u8p))
    if rc:
        raise BackendError(rc, "zl_test_fq2_sqrt")
    return out, ok[:n].astype(bool)


def hook_point_op(be: Optional["Backend"], group: int, hot: bool, op: int, pq: np.ndarray) -> np.ndarray:
    """pq: (n, 8, W) uint32 raw limbs of two XYZZ points (W = 14 for G1, 28 for G2) -> (n, 4, W)"""
    a = np.ascontiguousarray(pq, dtype=np.uint32)
    n, W = a.shape[0], a.shape[2]
    out = np.zeros((n, 4, W), dtype=np.uint32)
    L = load_library()
    rc = L.zl_test_point_op(be._ctx if be is not None else None, group, int(hot), op, _p32(a), n, _p32(out))
    if rc:
        raise BackendError(rc, "zl_test_point_op")
    return out


# forms of zl_test_point_form_op (include/zl_backend_test.h)
FORM_SCALAR, FORM_SCALAR_HOT, FORM_QUAD, FORM_PAIR, FORM_OCTET = 0, 1, 2, 3, 4


def hook_fp2pair_op(be: "Backend", curve: int, op: int, operands: np.ndarray) -> np.ndarray:
    """Fq2 on a lane pair (Fp2H, device only): operands (n, 4, 2 L) uint32 raw limbs, c0 || c1 -> (n, 2 L); L = 14 (BLS12-381) or 10 (BN254)"""
    a = np.ascontiguousarray(operands, dtype=np.uint32)
    n, W = a.shape[0], (28 if curve == ZL_BLS12_381 else 20)
    assert a.shape[1:] == (4, W)
    out = np.zeros((n, W), dtype=np.uint32)
    rc = load_library().zl_test_fp2pair_op(be._ctx if be is not None else None, curve, op, _p32(a), n, _p32(out))
    if rc:
        raise BackendError(rc, "zl_test_fp2pair_op")
    return out


def hook_point_form_op(be: Optional["Backend"], curve: int, group: int, form: int, op: int, pq: np.ndarray) -> np.ndarray:
    """pq: (n, 8, W) uint32 raw limbs of two XYZZ points (W = L for G1, 2 L for G2) -> (n, 4, W), through the given form of the point formulas;
    be = None runs the host code path (scalar forms only)"""
    a = np.ascontiguousarray(pq, dtype=np.uint32)
    n, W = a.shape[0], a.shape[2]
    assert a.shape[1] == 8 and W == (14 if curve == ZL_BLS12_381 else 10) * (1 if group == ZL_G1 else 2)
    out = np.zeros((n, 4, W), dtype=np.uint32)
    rc = load_library().zl_test_point_form_op(be._ctx if be is not None else None, curve, group, form, op, _p32(a), n, _p32(out))
    if rc:
        raise BackendError(rc, "zl_test_point_form_op")
    return out


def hook_fr28_op(be: Optional["Backend"], curve: int, op: int, ab: np.ndarray, j: int = 2, bits: int = 28) -> np.ndarray:
    """ab: (n, 2, 8) uint32 words of two values < 2^256 -> (n, 8) canonical result words; be = None runs the host code path;
    bits = 28: the 10 x 28-bit instance (R' = 2^280), 29: the 9 x 29-bit instance (R' = 2^261)"""
    a = np.ascontiguousarray(ab, dtype=np.uint32)
    n = a.shape[0]
    out = np.zeros((n, 8), dtype=np.uint32)
    L = load_library()
    fn = L.zl_test_fr28_op if bits == 28 else L.zl_test_fr29_op
    rc = fn(be._ctx if be is not None else None, curve, op, j, _p32(a), n, _p32(out))
    if rc:
        raise BackendError(rc, "zl_test_fr28_op" if bits == 28 else "zl_test_fr29_op")
    return out


FP_FIELD_WORDS = {0: 8, 1: 12, 2: 8, 3: 8}  # zl_test_fp_op: BLS12-381 Fr, BLS12-381 Fq, BN254 Fr, BN254 Fq


def hook_fp_op(be: Optional["Backend"], field: int, form: int, op: int, abcd: np.ndarray, n: Optional[int] = None, out: Optional[np.ndarray] = None) -> np.ndarray:
    """the carry-chain field Fp<P> / Fp2<P> on raw words (zl_test_fp_op): abcd (n, 4, N) uint32 -> (n, N), or (n, 2 N) for the Fp2 ops (op >= 20);
    form 0 zl::mul as the unit builds it, 1 mul_impl, 2 mul_body; be = None runs the host code.  n: the records to process (default all);
    out: a caller's buffer of at least n rows, written in place (rows from n on are the caller's to inspect)"""
    a = np.ascontiguousarray(abcd, dtype=np.uint32)
    N = FP_FIELD_WORDS.get(field, 8)
    n = a.shape[0] if n is None else n
    assert a.ndim == 3 and a.shape[1:] == (4, N) and n <= a.shape[0]
    W = 2 * N if op >= 20 else N
    if out is None:
        out = np.zeros((n, W), dtype=np.uint32)
    assert out.dtype == np.uint32 and out.flags["C_CONTIGUOUS"] and out.shape[0] >= n and out.shape[1] == W
    rc = load_library().zl_test_fp_op(be._ctx if be is not None else None, field, form, op, _p32(a), n, _p32(out))
    if rc:
        raise BackendError(rc, "zl_test_fp_op")
    return out


def hook_fq_mul_rate(be: "Backend", waves_per_simd: int = 3, iters: int = 3000) -> float:
    """10^9 Montgomery products per second of the accumulation kernel's multiplier on per-lane pseudo-random operands (measurement hook)"""
    v = C.c_double(0.0)
    be._check(be.L.zl_test_fq_mul_rate(be._ctx, waves_per_simd, iters, C.byref(v)), "zl_test_fq_mul_rate")
    return v.value


_CLOCK_KEYS = ("effective_clock_ghz", "span_ms_by_100mhz_counter", "waves", "mean_wave_life_ms", "min_wave_ghz", "max_wave_ghz")


def hook_fq_mul_clock(be: "Backend", waves_per_simd: int = 3, iters: int = 50000) -> dict:
    """effective shader clock of the multiplier chain (s_memtime / s_memrealtime per wave) + its rate in the same launch (measurement hook)"""
    v = (C.c_double * 8)()
    be._check(be.L.zl_test_fq_mul_clock(be._ctx, waves_per_simd, iters, v), "zl_test_fq_mul_clock")
    d = {k: float(v[i]) for i, k in enumerate(_CLOCK_KEYS)}
    d["g_products_per_s"] = float(v[6])
    d["ms_by_hip_events"] = float(v[7])
    return d


def hook_clock_probe_launch(be: "Backend", spin_us: int) -> None:
    """start the sleeping clock probe (one wave per XCD, own stream) for spin_us microseconds; launch the work to observe right after"""
    be._check(be.L.zl_test_clock_probe_launch(be._ctx, int(spin_us)), "zl_test_clock_probe_launch")


def hook_clock_probe_read(be: "Backend") -> dict:
    v = (C.c_double * 6)()
    be._check(be.L.zl_test_clock_probe_read(be._ctx, v), "zl_test_clock_probe_read")
    return {k: float(v[i]) for i, k in enumerate(_CLOCK_KEYS)}


def hook_acc_clock(be: "Backend", on: bool) -> None:
    """arm / disarm the clock-reading build of the large G1 accumulation kernel on this ctx (measurement hook)"""
    be._check(be.L.zl_test_acc_clock(be._ctx, 1 if on else 0), "zl_test_acc_clock")


def hook_acc_clock_read(be: "Backend") -> dict:
    v = (C.c_double * 6)()
    be._check(be.L.zl_test_acc_clock_read(be._ctx, v), "zl_test_acc_clock_read")
    return {k: float(v[i]) for i, k in enumerate(_CLOCK_KEYS)}


# ---- host mirror (openzl::R1CS / poseidon / Groth16<E>, csrc/zl_host.h) through its C hooks ---------------------------
def poseidon_permute(curve: int, state: np.ndarray) -> np.ndarray:
    """native Poseidon permutation on canonical (W,4) uint64 limbs, W in 3..6 (host code, no GPU)."""
    st = np.ascontiguousarray(np.array(state, dtype=np.uint64, copy=True))
    if st.size == 12:  # (width 3: the shapes this function always took)
        rc, what = load_library().zl_poseidon_permute(curve, _p64(st)), "zl_poseidon_permute"
    else:
        if st.ndim != 2 or st.shape[1] != 4:
            raise ValueError("a state is (W, 4) uint64 words")
        rc, what = load_library().zl_poseidon_permute_w(curve, st.shape[0], _p64(st)), "zl_poseidon_permute_w"
    if rc:
        raise BackendError(rc, what)
    return st


def poseidon_spec(arity: int) -> dict:
    """width, full_rounds, partial_rounds and tag of an arity in 2..5 (zl_poseidon_spec)"""
    w, rf, rp, tag = C.c_uint(), C.c_uint(), C.c_uint(), C.c_uint64()
    rc = load_library().zl_poseidon_spec(arity, C.byref(w), C.byref(rf), C.byref(rp), C.byref(tag))
    if rc:
        raise BackendError(rc, "zl_poseidon_spec")
    return {"arity": arity, "width": w.value, "full_rounds": rf.value, "partial_rounds": rp.value, "tag": tag.value}


def poseidon_constants(curve: int, width: int):
    """the generated constants of a width in 3..6, canonical: (width * rounds, 4) round keys and (width, width, 4) MDS entries (zl_poseidon_constants)"""
    L = load_library()
    if not 3 <= width <= 6:
        raise BackendError(-1, "zl_poseidon_constants")
    sp = poseidon_spec(width - 1)
    keys = np.zeros((width * (sp["full_rounds"] + sp["partial_rounds"]), 4), dtype=np.uint64)
    mds = np.zeros((width, width, 4), dtype=np.uint64)
    _pos_check(L, L.zl_poseidon_constants(curve, width, _p64(keys), _p64(mds)), "zl_poseidon_constants")
    return keys, mds


# ---- batched Poseidon: one implementation per call for Backend (its ctx) and for the host forms below (ctx == NULL: host thread pool, no device) ----
def _pos_check(L, rc: int, what: str):
    if rc != 0:
        raise BackendError(rc, what, L.zl_strerror(rc).decode())


def _elems(a, per: int) -> np.ndarray:
    """contiguous (count, per, 4) uint64 copy-or-view of canonical field elements"""
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64).reshape(-1, per, 4))


def _ptr_or_none(a: np.ndarray):
    return _p64(a) if a.size else None


def _poseidon_permute_batch(L, ctx, curve: int, states) -> np.ndarray:
    a = np.asarray(states, dtype=np.uint64)
    if a.ndim == 3 and a.shape[2] == 4 and a.shape[1] != 3:  # (count, W, 4): the width is the array's; every other shape is width-3 states as before
        st = np.ascontiguousarray(a).copy()
        _pos_check(L, L.zl_poseidon_permute_batch_w(ctx, curve, st.shape[1], _ptr_or_none(st), st.shape[0]), "zl_poseidon_permute_batch_w")
        return st
    st = _elems(states, 3).copy()
    _pos_check(L, L.zl_poseidon_permute_batch(ctx, curve, _ptr_or_none(st), st.shape[0]), "zl_poseidon_permute_batch")
    return st


def _poseidon_hash(L, ctx, curve: int, inputs) -> np.ndarray:
    v = np.ascontiguousarray(np.asarray(inputs, dtype=np.uint64))
    if v.ndim != 3 or v.shape[2] != 4:
        raise ValueError("inputs are (count, arity, 4) uint64 words")
    out = np.zeros((v.shape[0], 4), dtype=np.uint64)
    _pos_check(L, L.zl_poseidon_hash_batch(ctx, curve, v.shape[1], _ptr_or_none(v), v.shape[0], _ptr_or_none(out)), "zl_poseidon_hash_batch")
    return out


def _duplex_state(initial_state, width: int):
    if initial_state is None:
        return None
    st = np.ascontiguousarray(np.asarray(initial_state, dtype=np.uint64))
    if st.shape != (width, 4):
        raise ValueError("initial_state is (W, 4) uint64 words")
    return st


def _duplex_operands(keys, headers, texts):
    t = np.ascontiguousarray(np.asarray(texts, dtype=np.uint64))
    k = np.ascontiguousarray(np.asarray(keys, dtype=np.uint64))
    h = np.ascontiguousarray(np.asarray(headers, dtype=np.uint64))
    if t.ndim != 4 or t.shape[3] != 4 or k.ndim != 3 or h.ndim != 3 or k.shape[2] != 4 or h.shape[2] != 4 or not k.shape[0] == h.shape[0] == t.shape[0]:
        raise ValueError("texts are (count, N, W - 1, 4), keys (count, K, 4), headers (count, H, 4) uint64 words")
    return k, h, t


def _poseidon_duplex(L, ctx, curve: int, initial_state, keys, headers, texts, tags):
    """tags None: encrypt -> (ciphertexts, tags); otherwise decrypt -> (plaintexts, ok)"""
    k, h, t = _duplex_operands(keys, headers, texts)
    count, blocks, width = t.shape[0], t.shape[1], t.shape[2] + 1
    st = _duplex_state(initial_state, width)
    stp = None if st is None else _p64(st)
    out = np.zeros_like(t)
    if tags is None:
        tg = np.zeros((count, 4), dtype=np.uint64)
        _pos_check(L, L.zl_poseidon_duplex_encrypt_batch(ctx, curve, width, stp, _ptr_or_none(k), k.shape[1], _ptr_or_none(h), h.shape[1], _ptr_or_none(t), blocks, count,
                                                         _ptr_or_none(out), _ptr_or_none(tg)), "zl_poseidon_duplex_encrypt_batch")
        return out, tg
    tg = np.ascontiguousarray(np.asarray(tags, dtype=np.uint64).reshape(count, 4))
    ok = np.zeros(count, dtype=np.uint8)
    _pos_check(L, L.zl_poseidon_duplex_decrypt_batch(ctx, curve, width, stp, _ptr_or_none(k), k.shape[1], _ptr_or_none(h), h.shape[1], _ptr_or_none(t), _ptr_or_none(tg),
                                                     blocks, count, _ptr_or_none(out), ok.ctypes.data_as(C.POINTER(C.c_uint8)) if count else None),
               "zl_poseidon_duplex_decrypt_batch")
    return out, ok.astype(bool)


def _poseidon_encrypt_assignments(L, ctx, curve: int, initial_state, keys, headers, plaintexts) -> np.ndarray:
    k, h, t = _duplex_operands(keys, headers, plaintexts)
    count, blocks, width = t.shape[0], t.shape[1], t.shape[2] + 1
    st = _duplex_state(initial_state, width)
    out = np.zeros((count, L.zl_poseidon_encrypt_assignment_elems(width, k.shape[1], h.shape[1], blocks), 4), dtype=np.uint64)
    _pos_check(L, L.zl_poseidon_encrypt_assignments(ctx, curve, width, None if st is None else _p64(st), _ptr_or_none(k), k.shape[1], _ptr_or_none(h), h.shape[1],
                                                    _ptr_or_none(t), blocks, count, _ptr_or_none(out)), "zl_poseidon_encrypt_assignments")
    return out


def poseidon_encrypt_assignment_elems(width: int, key_len: int, header_len: int, blocks: int) -> int:
    """elements of one encryption's assignment: 2 + 2 N (W - 1) + H + K + 3 S (0 for a parameter out of range)"""
    if min(width, key_len, header_len, blocks) < 0:
        return 0
    return int(load_library().zl_poseidon_encrypt_assignment_elems(width, key_len, header_len, blocks))


def poseidon_encrypt_assignments_host(curve: int, initial_state, keys, headers, plaintexts) -> np.ndarray:
    return _poseidon_encrypt_assignments(load_library(), None, curve, initial_state, keys, headers, plaintexts)


def poseidon_duplex_permutations(width: int, key_len: int, header_len: int, blocks: int) -> int:
    """dependent permutations per message: key_len // rate + 1 + header_len // rate + 1 + blocks (0 for a parameter out of range)"""
    if min(width, key_len, header_len, blocks) < 0:
        return 0
    return int(load_library().zl_poseidon_duplex_permutations(width, key_len, header_len, blocks))


def poseidon_duplex_encrypt_host(curve: int, initial_state, keys, headers, plaintexts):
    return _poseidon_duplex(load_library(), None, curve, initial_state, keys, headers, plaintexts, None)


def poseidon_duplex_decrypt_host(curve: int, initial_state, keys, headers, ciphertexts, tags):
    return _poseidon_duplex(load_library(), None, curve, initial_state, keys, headers, ciphertexts, tags)


# ---- the embedded twisted Edwards curves and hybrid encryption (zl_ed_*, zl_hybrid_*) ---------------------------------------------------------------------
def _u8p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint8)) if a.size else None


def _ed_operand(a, per: int, what: str):
    """(count, per, 4) words and stride 1 -- scalars also as (count, 4) --, or ONE operand and stride 0: a point (2, 4), a scalar (4,).  A (1, 4) scalar array is
    a batch of one, not the broadcast form."""
    v = np.ascontiguousarray(np.asarray(a, dtype=np.uint64))
    if v.shape == ((4,) if per == 1 else (per, 4)):
        return v.reshape(1, per, 4), 0
    if per == 1 and v.ndim == 2 and v.shape[1] == 4:
        v = v.reshape(-1, 1, 4)
    if v.ndim != 3 or v.shape[1:] != (per, 4):
        raise ValueError(f"{what} are (count, {per}, 4) uint64 words, or one operand for all items")
    return v, 1


def _ed_count(*ops):
    counts = {v.shape[0] for v, stride in ops if stride}
    if len(counts) > 1:
        raise ValueError("operands of different counts")
    return counts.pop() if counts else 1


def ed_params(curve: int) -> dict:
    """zl_ed_params: {"a", "d", "order", "cofactor"} of the embedded curve a x^2 + y^2 = 1 + d x^2 y^2 over `curve`'s scalar field, as Python integers"""
    L = load_library()
    out = np.zeros((4, 4), dtype=np.uint64)
    _pos_check(L, L.zl_ed_params(curve, _p64(out[0]), _p64(out[1]), _p64(out[2]), _p64(out[3])), "zl_ed_params")
    vals = [sum(int(w) << (64 * i) for i, w in enumerate(row)) for row in out]
    return dict(zip(("a", "d", "order", "cofactor"), vals))


def ed_add_host(curve: int, p, q) -> np.ndarray:
    """zl_ed_add: p + q for two points (2, 4) of the embedded curve -> (2, 4)"""
    L = load_library()
    a = np.ascontiguousarray(np.asarray(p, dtype=np.uint64).reshape(2, 4))
    b = np.ascontiguousarray(np.asarray(q, dtype=np.uint64).reshape(2, 4))
    out = np.zeros((2, 4), dtype=np.uint64)
    _pos_check(L, L.zl_ed_add(curve, _p64(a), _p64(b), _p64(out)), "zl_ed_add")
    return out


def _ed_scalar_mul(L, ctx, curve: int, points, scalars, check_subgroup: bool):
    (p, ps), (k, ks) = _ed_operand(points, 2, "points"), _ed_operand(scalars, 1, "scalars")
    count = _ed_count((p, ps), (k, ks))
    out = np.zeros((count, 2, 4), dtype=np.uint64)
    status = np.zeros(count, dtype=np.uint8)
    _pos_check(L, L.zl_ed_scalar_mul_batch(ctx, curve, _p64(p), ps, _p64(k), ks, count, ZL_ED_CHECK_SUBGROUP if check_subgroup else 0, _p64(out), _u8p(status)),
               "zl_ed_scalar_mul_batch")
    return out, status


def ed_scalar_mul_host(curve: int, points, scalars, check_subgroup: bool = False):
    """Backend.ed_scalar_mul on the host mirror"""
    return _ed_scalar_mul(load_library(), None, curve, points, scalars, check_subgroup)


def ed_order_bits(curve: int) -> int:
    """bit length of the embedded curve's subgroup order: the full width of a scalar-multiplication circuit (252 Jubjub, 251 Baby Jubjub)"""
    return ed_params(curve)["order"].bit_length()


def ed_scalar_mul_assignment_elems(curve: int, bits: int) -> int:
    """elements of one scalar-multiplication assignment: 14 bits - 5 (0 for a parameter out of range)"""
    if not 0 <= bits < 2**32:
        return 0
    return int(load_library().zl_ed_scalar_mul_assignment_elems(curve, bits))


def _ed_scalar_mul_assignments(L, ctx, curve: int, points, scalars, bits) -> np.ndarray:
    (p, ps), k = _ed_operand(points, 2, "points"), np.ascontiguousarray(np.asarray(scalars, dtype=np.uint64)).reshape(-1, 4)
    count = k.shape[0]
    if ps and p.shape[0] != count:
        raise ValueError("operands of different counts")
    bits = ed_order_bits(curve) if bits is None else bits
    out = np.zeros((count, ed_scalar_mul_assignment_elems(curve, bits), 4), dtype=np.uint64)
    _pos_check(L, L.zl_ed_scalar_mul_assignments(ctx, curve, bits, _p64(p), ps, _ptr_or_none(k), count, _ptr_or_none(out)), "zl_ed_scalar_mul_assignments")
    return out


def ed_scalar_mul_assignments_host(curve: int, points, scalars, bits=None) -> np.ndarray:
    """Backend.ed_scalar_mul_assignments on the host mirror"""
    return _ed_scalar_mul_assignments(load_library(), None, curve, points, scalars, bits)


def _hybrid_operands(initial_state, generator, esk, pks, headers, plaintexts):
    t = np.ascontiguousarray(np.asarray(plaintexts, dtype=np.uint64))
    h = np.ascontiguousarray(np.asarray(headers, dtype=np.uint64))
    if t.ndim != 4 or t.shape[3] != 4 or h.ndim != 3 or h.shape[2] != 4 or h.shape[0] != t.shape[0]:
        raise ValueError("plaintexts are (count, N, W - 1, 4), headers (count, H, 4) uint64 words")
    count = t.shape[0]
    g = np.ascontiguousarray(np.asarray(generator, dtype=np.uint64).reshape(2, 4))
    e = np.ascontiguousarray(np.asarray(esk, dtype=np.uint64).reshape(count, 4))
    pk, ps = _ed_operand(pks, 2, "pks")
    if ps and pk.shape[0] != count:
        raise ValueError("one public key per item, or one for all")
    return _duplex_state(initial_state, t.shape[2] + 1), g, e, pk, ps, h, t


def hybrid_encrypt_assignment_elems(curve: int, width: int, bits: int, header_len: int, blocks: int) -> int:
    """elements of one hybrid-encryption assignment: 27 bits - 13 + 2 N (W - 1) + H + 3 S (0 for a parameter out of range)"""
    if not (0 <= width < 2**32 and 0 <= bits < 2**32 and 0 <= header_len < 2**63 and 0 <= blocks < 2**63):
        return 0
    return int(load_library().zl_hybrid_encrypt_assignment_elems(curve, width, bits, header_len, blocks))


def _hybrid_encrypt_assignments(L, ctx, curve: int, initial_state, generator, esk, pks, headers, plaintexts, bits) -> np.ndarray:
    st, g, e, pk, ps, h, t = _hybrid_operands(initial_state, generator, esk, pks, headers, plaintexts)
    count, blocks, width = t.shape[0], t.shape[1], t.shape[2] + 1
    bits = ed_order_bits(curve) if bits is None else bits
    out = np.zeros((count, hybrid_encrypt_assignment_elems(curve, width, bits, h.shape[1], blocks), 4), dtype=np.uint64)
    _pos_check(L, L.zl_hybrid_encrypt_assignments(ctx, curve, width, bits, None if st is None else _p64(st), _p64(g), _ptr_or_none(e), _p64(pk), ps, _ptr_or_none(h),
                                                  h.shape[1], _ptr_or_none(t), blocks, count, _ptr_or_none(out)), "zl_hybrid_encrypt_assignments")
    return out


def hybrid_encrypt_assignments_host(curve: int, initial_state, generator, esk, pks, headers, plaintexts, bits=None) -> np.ndarray:
    """Backend.hybrid_encrypt_assignments on the host mirror"""
    return _hybrid_encrypt_assignments(load_library(), None, curve, initial_state, generator, esk, pks, headers, plaintexts, bits)


def _hybrid_encrypt(L, ctx, curve: int, initial_state, generator, esk, pks, headers, plaintexts, check_subgroup: bool):
    t = np.ascontiguousarray(np.asarray(plaintexts, dtype=np.uint64))
    h = np.ascontiguousarray(np.asarray(headers, dtype=np.uint64))
    if t.ndim != 4 or t.shape[3] != 4 or h.ndim != 3 or h.shape[2] != 4 or h.shape[0] != t.shape[0]:
        raise ValueError("plaintexts are (count, N, W - 1, 4), headers (count, H, 4) uint64 words")
    count, blocks, width = t.shape[0], t.shape[1], t.shape[2] + 1
    g = np.ascontiguousarray(np.asarray(generator, dtype=np.uint64).reshape(2, 4))
    e = np.ascontiguousarray(np.asarray(esk, dtype=np.uint64).reshape(count, 4))
    pk, ps = _ed_operand(pks, 2, "pks")
    if ps and pk.shape[0] != count:
        raise ValueError("one public key per item, or one for all")
    st = _duplex_state(initial_state, width)
    epks, out, tags, status = np.zeros((count, 2, 4), dtype=np.uint64), np.zeros_like(t), np.zeros((count, 4), dtype=np.uint64), np.zeros(count, dtype=np.uint8)
    _pos_check(L, L.zl_hybrid_encrypt_batch(ctx, curve, width, None if st is None else _p64(st), _p64(g), _ptr_or_none(e), _p64(pk), ps, _ptr_or_none(h), h.shape[1],
                                            _ptr_or_none(t), blocks, count, ZL_ED_CHECK_SUBGROUP if check_subgroup else 0, _ptr_or_none(epks), _ptr_or_none(out),
                                            _ptr_or_none(tags), _u8p(status)), "zl_hybrid_encrypt_batch")
    return epks, out, tags, status


def _hybrid_decrypt(L, ctx, curve: int, initial_state, sks, epks, headers, ciphertexts, tags, check_subgroup: bool):
    t = np.ascontiguousarray(np.asarray(ciphertexts, dtype=np.uint64))
    h = np.ascontiguousarray(np.asarray(headers, dtype=np.uint64))
    if t.ndim != 4 or t.shape[3] != 4 or h.ndim != 3 or h.shape[2] != 4 or h.shape[0] != t.shape[0]:
        raise ValueError("ciphertexts are (count, N, W - 1, 4), headers (count, H, 4) uint64 words")
    count, blocks, width = t.shape[0], t.shape[1], t.shape[2] + 1
    sk, ks = _ed_operand(sks, 1, "sks")
    if ks and sk.shape[0] != count:
        raise ValueError("one secret key per item, or one for all")
    ep = np.ascontiguousarray(np.asarray(epks, dtype=np.uint64).reshape(count, 2, 4))
    tg = np.ascontiguousarray(np.asarray(tags, dtype=np.uint64).reshape(count, 4))
    st = _duplex_state(initial_state, width)
    out, ok, status = np.zeros_like(t), np.zeros(count, dtype=np.uint8), np.zeros(count, dtype=np.uint8)
    _pos_check(L, L.zl_hybrid_decrypt_batch(ctx, curve, width, None if st is None else _p64(st), _p64(sk), ks, _ptr_or_none(ep), _ptr_or_none(h), h.shape[1],
                                            _ptr_or_none(t), _ptr_or_none(tg), blocks, count, ZL_ED_CHECK_SUBGROUP if check_subgroup else 0, _ptr_or_none(out),
                                            _u8p(ok), _u8p(status)), "zl_hybrid_decrypt_batch")
    return out, ok.astype(bool), status


def hybrid_encrypt_host(curve: int, initial_state, generator, esk, pks, headers, plaintexts, check_subgroup: bool = False):
    return _hybrid_encrypt(load_library(), None, curve, initial_state, generator, esk, pks, headers, plaintexts, check_subgroup)


def hybrid_decrypt_host(curve: int, initial_state, sks, epks, headers, ciphertexts, tags, check_subgroup: bool = False):
    return _hybrid_decrypt(load_library(), None, curve, initial_state, sks, epks, headers, ciphertexts, tags, check_subgroup)


def _poseidon_hash2(L, ctx, curve: int, xy) -> np.ndarray:
    v = _elems(xy, 2)
    out = np.zeros((v.shape[0], 4), dtype=np.uint64)
    _pos_check(L, L.zl_poseidon_hash2_batch(ctx, curve, _ptr_or_none(v), v.shape[0], _ptr_or_none(out)), "zl_poseidon_hash2_batch")
    return out


def _poseidon_chain(L, ctx, curve: int, x0, x1, k: int) -> np.ndarray:
    a, b = _elems(x0, 1), _elems(x1, 1)
    assert a.shape == b.shape
    out = np.zeros((a.shape[0], 4), dtype=np.uint64)
    _pos_check(L, L.zl_poseidon_chain_batch(ctx, curve, _ptr_or_none(a), _ptr_or_none(b), k, a.shape[0], _ptr_or_none(out)), "zl_poseidon_chain_batch")
    return out


def _poseidon_chain_assignments(L, ctx, curve: int, x0, x1, k: int) -> np.ndarray:
    a, b = _elems(x0, 1), _elems(x1, 1)
    assert a.shape == b.shape
    out = np.zeros((a.shape[0], L.zl_poseidon_chain_assignment_elems(k), 4), dtype=np.uint64)
    _pos_check(L, L.zl_poseidon_chain_assignments(ctx, curve, _ptr_or_none(a), _ptr_or_none(b), k, a.shape[0], _ptr_or_none(out)), "zl_poseidon_chain_assignments")
    return out


def _poseidon_merkle_root(L, ctx, curve: int, leaves, depth: int) -> np.ndarray:
    lv = _elems(leaves, 1)
    root = np.zeros(4, dtype=np.uint64)
    _pos_check(L, L.zl_poseidon_merkle_root(ctx, curve, _ptr_or_none(lv), lv.shape[0], depth, _p64(root)), "zl_poseidon_merkle_root")
    return root


def _poseidon_merkle_build(L, ctx, curve: int, leaves, depth: int):
    lv = _elems(leaves, 1)
    nodes = np.zeros((L.zl_poseidon_merkle_nodes(lv.shape[0], depth), 4), dtype=np.uint64)
    root = np.zeros(4, dtype=np.uint64)
    _pos_check(L, L.zl_poseidon_merkle_build(ctx, curve, _ptr_or_none(lv), lv.shape[0], depth, _ptr_or_none(nodes), _p64(root)), "zl_poseidon_merkle_build")
    return nodes, root


def _poseidon_roots_from_paths(L, ctx, curve: int, leaves, indices, paths, depth: int) -> np.ndarray:
    lv = _elems(leaves, 1)
    idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
    pa = np.ascontiguousarray(np.asarray(paths, dtype=np.uint64).reshape(-1, depth, 4))
    assert lv.shape[0] == idx.size == pa.shape[0]
    roots = np.zeros((idx.size, 4), dtype=np.uint64)
    _pos_check(L, L.zl_poseidon_merkle_roots_from_paths(ctx, curve, _ptr_or_none(lv), _ptr_or_none(idx), _ptr_or_none(pa), depth, idx.size, _ptr_or_none(roots)),
               "zl_poseidon_merkle_roots_from_paths")
    return roots


def _poseidon_merkle_assignments(L, ctx, curve: int, leaves, indices, paths, depth: int) -> np.ndarray:
    lv = _elems(leaves, 1)
    idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
    pa = np.ascontiguousarray(np.asarray(paths, dtype=np.uint64).reshape(-1, max(1, depth), 4))
    assert lv.shape[0] == idx.size == pa.shape[0]
    out = np.zeros((idx.size, L.zl_poseidon_merkle_assignment_elems(depth), 4), dtype=np.uint64)
    _pos_check(L, L.zl_poseidon_merkle_assignments(ctx, curve, _ptr_or_none(lv), _ptr_or_none(idx), _ptr_or_none(pa), depth, idx.size, _ptr_or_none(out)),
               "zl_poseidon_merkle_assignments")
    return out


def poseidon_merkle_assignment_elems(depth: int) -> int:
    """elements of one membership's assignment: 3 + 238 depth (0 for a depth outside 1..40)"""
    return int(load_library().zl_poseidon_merkle_assignment_elems(depth))


def poseidon_merkle_assignments_host(curve: int, leaves, indices, paths, depth: int) -> np.ndarray:
    return _poseidon_merkle_assignments(load_library(), None, curve, leaves, indices, paths, depth)


# arity -> 3 S(arity): the record elements of one in-circuit hash (x^2, x^4, x^5 of 8 (arity + 1) + partial - 1 S-boxes)
_ARITY_RECORDS = {2: 234, 3: 258, 4: 285, 5: 309}


def _arity_inputs(inputs) -> np.ndarray:
    v = np.ascontiguousarray(np.asarray(inputs, dtype=np.uint64))
    if v.ndim != 3 or v.shape[2] != 4:
        raise ValueError("inputs are (count, arity, 4) uint64 words")
    return v


def _poseidon_hash_assignments(L, ctx, curve: int, inputs) -> np.ndarray:
    v = _arity_inputs(inputs)
    out = np.zeros((v.shape[0], L.zl_poseidon_hash_assignment_elems(v.shape[1]), 4), dtype=np.uint64)
    _pos_check(L, L.zl_poseidon_hash_assignments(ctx, curve, v.shape[1], _ptr_or_none(v), v.shape[0], _ptr_or_none(out)), "zl_poseidon_hash_assignments")
    return out


def _poseidon_merkle_leaf_assignments(L, ctx, curve: int, preimages, indices, paths, depth: int) -> np.ndarray:
    pre = _arity_inputs(preimages)
    idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
    pa = np.ascontiguousarray(np.asarray(paths, dtype=np.uint64).reshape(-1, max(1, depth), 4))
    assert pre.shape[0] == idx.size == pa.shape[0]
    out = np.zeros((idx.size, L.zl_poseidon_merkle_leaf_assignment_elems(pre.shape[1], depth), 4), dtype=np.uint64)
    _pos_check(L, L.zl_poseidon_merkle_leaf_assignments(ctx, curve, pre.shape[1], _ptr_or_none(pre), _ptr_or_none(idx), _ptr_or_none(pa), depth, idx.size,
                                                        _ptr_or_none(out)), "zl_poseidon_merkle_leaf_assignments")
    return out


def poseidon_hash_assignment_elems(arity: int) -> int:
    """elements of one hash circuit's assignment: 2 + arity + 3 S(arity) = 238, 263, 291, 316 (0 for an arity outside 2..5)"""
    return int(load_library().zl_poseidon_hash_assignment_elems(arity))


def poseidon_merkle_leaf_assignment_elems(arity: int, depth: int) -> int:
    """elements of one leaf membership's assignment: poseidon_hash_assignment_elems(arity) + 238 depth (0 for a parameter out of range)"""
    return int(load_library().zl_poseidon_merkle_leaf_assignment_elems(arity, depth))


def poseidon_hash_assignments_host(curve: int, inputs) -> np.ndarray:
    return _poseidon_hash_assignments(load_library(), None, curve, inputs)


def poseidon_merkle_leaf_assignments_host(curve: int, preimages, indices, paths, depth: int) -> np.ndarray:
    return _poseidon_merkle_leaf_assignments(load_library(), None, curve, preimages, indices, paths, depth)


def poseidon_merkle_nodes(n: int, depth: int) -> int:
    """elements of the node array of a tree over n leaves with `depth` hash levels (0 for an invalid shape)"""
    return int(load_library().zl_poseidon_merkle_nodes(n, depth))


def poseidon_permute_batch_host(curve: int, states) -> np.ndarray:
    return _poseidon_permute_batch(load_library(), None, curve, states)


def poseidon_hash2_host(curve: int, xy) -> np.ndarray:
    return _poseidon_hash2(load_library(), None, curve, xy)


def poseidon_hash_host(curve: int, inputs) -> np.ndarray:
    return _poseidon_hash(load_library(), None, curve, inputs)


def poseidon_chain_host(curve: int, x0, x1, k: int) -> np.ndarray:
    return _poseidon_chain(load_library(), None, curve, x0, x1, k)


def poseidon_chain_assignment_elems(k: int) -> int:
    """elements of one chain's assignment: 4 + 234 k (0 for k == 0 or a variable count that does not fit 31 bits)"""
    return int(load_library().zl_poseidon_chain_assignment_elems(k))


def poseidon_chain_assignments_host(curve: int, x0, x1, k: int) -> np.ndarray:
    return _poseidon_chain_assignments(load_library(), None, curve, x0, x1, k)


def poseidon_merkle_root_host(curve: int, leaves, depth: int) -> np.ndarray:
    return _poseidon_merkle_root(load_library(), None, curve, leaves, depth)


def poseidon_merkle_build_host(curve: int, leaves, depth: int):
    return _poseidon_merkle_build(load_library(), None, curve, leaves, depth)


def poseidon_merkle_paths_host(nodes: np.ndarray, n: int, depth: int, indices) -> np.ndarray:
    """zl_poseidon_merkle_paths: the gather of Backend.poseidon_merkle_paths over a node array in host memory"""
    L = load_library()
    nd = _elems(nodes, 1)
    idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
    paths = np.zeros((max(1, idx.size), depth, 4), dtype=np.uint64)
    _pos_check(L, L.zl_poseidon_merkle_paths(_ptr_or_none(nd), n, depth, _ptr_or_none(idx), idx.size, _p64(paths)), "zl_poseidon_merkle_paths")
    return paths[: idx.size]


def poseidon_roots_from_paths_host(curve: int, leaves, indices, paths, depth: int) -> np.ndarray:
    return _poseidon_roots_from_paths(load_library(), None, curve, leaves, indices, paths, depth)


def _p32(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint32)) if a.size else None


def _forest_items(tree_of, indices):
    """(tree_of as contiguous uint32, indices as contiguous uint64), one entry per item"""
    tr = np.ascontiguousarray(tree_of, dtype=np.uint32).reshape(-1)
    idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
    if tr.size != idx.size:
        raise ValueError("tree_of and indices name the same items")
    return tr, idx


class MerkleForest:
    """zl_merkle_forest: `trees` growing Merkle trees of `depth` hash levels and room for `capacity` leaves each in one allocation -- device memory of `backend`
    (which must outlive the forest), or host memory when backend is None (the host mirror: same layout, same bytes, no device).  Tree t's node array has the
    layout of poseidon_merkle_build_dev for n = capacity, so tree_nodes(t) with n = capacity serves every (d_nodes, n, depth) entry point of Backend."""

    def __init__(self, backend: Optional[Backend], curve: int, trees: int, depth: int, capacity: int):
        self.L = backend.L if backend is not None else load_library()
        self.backend, self.curve = backend, curve
        self._f = C.c_void_p()
        self._check(self.L.zl_merkle_forest_create(backend._ctx if backend is not None else None, curve, trees, depth, capacity, C.byref(self._f)), "zl_merkle_forest_create")
        t, d, c, st = C.c_uint32(), C.c_uint(), C.c_size_t(), C.c_size_t()
        self._check(self.L.zl_merkle_forest_describe(self._f, C.byref(t), C.byref(d), C.byref(c), C.byref(st)), "zl_merkle_forest_describe")
        self.trees, self.depth, self.capacity, self.tree_stride = t.value, d.value, c.value, st.value

    def _check(self, rc: int, what: str):
        _pos_check(self.L, rc, what)

    def append(self, tree_of, leaves):
        """leaf i (host, (count, 4) canonical words) goes to tree tree_of[i], behind the leaves that tree already has, in input order"""
        tr = np.ascontiguousarray(tree_of, dtype=np.uint32).reshape(-1)
        lv = _elems(leaves, 1)
        if lv.shape[0] != tr.size:
            raise ValueError("one tree id per leaf")
        self._check(self.L.zl_merkle_forest_append(self._f, _p32(tr), _ptr_or_none(lv), tr.size), "zl_merkle_forest_append")

    def append_dev(self, tree_of, d_leaves: int, count: int):
        """append with the `count` leaves at the device address d_leaves (validated on the device before anything is written)"""
        tr = np.ascontiguousarray(tree_of, dtype=np.uint32).reshape(-1)
        if tr.size != count:
            raise ValueError("one tree id per leaf")
        self._check(self.L.zl_merkle_forest_append_dev(self._f, _p32(tr), C.c_void_p(d_leaves) if count else None, count), "zl_merkle_forest_append_dev")

    def lens(self) -> np.ndarray:
        out = np.zeros(self.trees, dtype=np.uint64)
        self._check(self.L.zl_merkle_forest_lens(self._f, _p64(out)), "zl_merkle_forest_lens")
        return out

    def roots(self) -> np.ndarray:
        out = np.zeros((self.trees, 4), dtype=np.uint64)
        self._check(self.L.zl_merkle_forest_roots(self._f, _p64(out)), "zl_merkle_forest_roots")
        return out

    def paths(self, tree_of, indices) -> np.ndarray:
        """(count, depth, 4): the siblings of leaf indices[i] of tree tree_of[i], bottom up"""
        tr, idx = _forest_items(tree_of, indices)
        out = np.zeros((max(1, idx.size), self.depth, 4), dtype=np.uint64)
        self._check(self.L.zl_merkle_forest_paths(self._f, _p32(tr), _ptr_or_none(idx), idx.size, _p64(out)), "zl_merkle_forest_paths")
        return out[: idx.size]

    def tree_nodes(self, tree: int) -> int:
        """the address of tree `tree`'s node array (device memory; host memory for the mirror)"""
        p = C.c_void_p()
        self._check(self.L.zl_merkle_forest_tree_nodes(self._f, tree, C.byref(p)), "zl_merkle_forest_tree_nodes")
        return p.value

    def download(self, tree: int) -> np.ndarray:
        """(tree_stride, 4): every node of one tree, in the capacity's layout"""
        out = np.zeros((self.tree_stride, 4), dtype=np.uint64)
        self._check(self.L.zl_merkle_forest_download(self._f, tree, _p64(out)), "zl_merkle_forest_download")
        return out

    def member_assignments_dev(self, tree_of, indices, d_out: int, stride_elems: Optional[int] = None):
        """zl_merkle_forest_member_assignments_dev: row i (at d_out + i * stride_elems elements; default the row length) = the membership of leaf indices[i] of
        tree tree_of[i], as Backend.poseidon_merkle_member_assignments_dev writes it for that tree"""
        tr, idx = _forest_items(tree_of, indices)
        stride = self.L.zl_poseidon_merkle_assignment_elems(self.depth) if stride_elems is None else stride_elems
        self._check(self.L.zl_merkle_forest_member_assignments_dev(self._f, _p32(tr), _ptr_or_none(idx), idx.size, C.c_void_p(d_out), stride),
                    "zl_merkle_forest_member_assignments_dev")

    def close(self):
        if self._f:
            self.L.zl_merkle_forest_destroy(self._f)
            self._f = C.c_void_p()

    def __enter__(self) -> "MerkleForest":
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pairing_product(backend: "Backend", curve: int, ps: np.ndarray, qs: np.ndarray) -> np.ndarray:
    """prod_i e(P_i, Q_i) with the Miller loops on backend's GPU (Backend.pairing_product)"""
    return backend.pairing_product(curve, ps, qs)


def pairing(curve: int, p_xy: np.ndarray, q_xy: np.ndarray) -> np.ndarray:
    """e(P, Q) as 12 canonical Fq coefficients (host pairing, no GPU)"""
    out = np.zeros((12, FQ_LIMBS[curve]), dtype=np.uint64)
    rc = load_library().zl_pairing(curve, _p64(np.ascontiguousarray(p_xy, dtype=np.uint64)), _p64(np.ascontiguousarray(q_xy, dtype=np.uint64)), _p64(out))
    if rc:
        raise BackendError(rc, "zl_pairing")
    return out


def _proof_struct(proof) -> "G16ProofC":
    pc = G16ProofC()
    a, ai, b, bi, c, ci = proof
    for i, v in enumerate(a):
        pc.a[i] = int(v)
    for i, v in enumerate(b):
        pc.b[i] = int(v)
    for i, v in enumerate(c):
        pc.c[i] = int(v)
    pc.a_inf, pc.b_inf, pc.c_inf = int(ai), int(bi), int(ci)
    return pc


def point_to_bytes(curve: int, group: int, xy: np.ndarray, inf: int = 0) -> bytes:
    """arkworks CanonicalSerialize (compressed) of one affine point given as canonical limbs (host code, no GPU)."""
    L = load_library()
    out = (C.c_uint8 * L.zl_point_bytes(curve, group))()
    rc = L.zl_point_to_bytes(curve, group, _p64(np.ascontiguousarray(xy, dtype=np.uint64)), int(inf), out)
    if rc:
        raise BackendError(rc, "zl_point_to_bytes")
    return bytes(out)


def point_from_bytes(curve: int, group: int, data: bytes):
    L = load_library()
    if len(data) != L.zl_point_bytes(curve, group):
        raise BackendError(-1, "zl_point_from_bytes", "wrong length")
    xy = np.zeros(2 * group * FQ_LIMBS[curve], dtype=np.uint64)
    inf = C.c_uint8(0)
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    rc = L.zl_point_from_bytes(curve, group, buf, _p64(xy), C.byref(inf))
    if rc:
        raise BackendError(rc, "zl_point_from_bytes")
    return xy, inf.value


def point_to_bytes_uncompressed(curve: int, group: int, xy: np.ndarray, inf: int = 0) -> bytes:
    """arkworks serialize_uncompressed of one affine point given as canonical limbs (host code, no GPU)."""
    L = load_library()
    out = (C.c_uint8 * L.zl_point_bytes_uncompressed(curve, group))()
    rc = L.zl_point_to_bytes_uncompressed(curve, group, _p64(np.ascontiguousarray(xy, dtype=np.uint64)), int(inf), out)
    if rc:
        raise BackendError(rc, "zl_point_to_bytes_uncompressed")
    return bytes(out)


def point_from_bytes_uncompressed(curve: int, group: int, data: bytes, check: bool = False):
    L = load_library()
    if len(data) != L.zl_point_bytes_uncompressed(curve, group):
        raise BackendError(-1, "zl_point_from_bytes_uncompressed", "wrong length")
    xy = np.zeros(2 * group * FQ_LIMBS[curve], dtype=np.uint64)
    inf = C.c_uint8(0)
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    rc = L.zl_point_from_bytes_uncompressed(curve, group, buf, int(check), _p64(xy), C.byref(inf))
    if rc:
        raise BackendError(rc, "zl_point_from_bytes_uncompressed")
    return xy, inf.value


def proof_to_bytes(curve: int, proof) -> bytes:
    """proof = (a, a_inf, b, b_inf, c, c_inf) as returned by Groth16Keys.prove -> 192 (BLS12-381) / 128 (BN254) bytes"""
    L = load_library()
    out = (C.c_uint8 * L.zl_groth16_proof_bytes(curve))()
    pc = _proof_struct(proof)
    rc = L.zl_groth16_proof_to_bytes(curve, C.byref(pc), out)
    if rc:
        raise BackendError(rc, "zl_groth16_proof_to_bytes")
    return bytes(out)


def proof_from_bytes(curve: int, data: bytes):
    L = load_library()
    pc = G16ProofC()
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data if data else b"\0")
    rc = L.zl_groth16_proof_from_bytes(curve, buf, len(data), C.byref(pc))
    if rc:
        raise BackendError(rc, "zl_groth16_proof_from_bytes")
    nq = FQ_LIMBS[curve]
    return (np.array(pc.a[: 2 * nq], dtype=np.uint64), pc.a_inf, np.array(pc.b[: 4 * nq], dtype=np.uint64), pc.b_inf,
            np.array(pc.c[: 2 * nq], dtype=np.uint64), pc.c_inf)


class Circuit:
    """R1CS<F> compiler in proof mode holding the config-5 Poseidon-chain circuit (host code, no GPU)."""

    def __init__(self, curve: int, k: int, x0: int = 1, x1: int = 2, witness_only: bool = False):
        """witness_only: run the circuit in a witness-only compiler (R1CS::for_witness: values, no rows) -- for proofs against keys that already hold the matrices"""
        self.L = load_library()
        self.curve = curve
        self.witness_only = witness_only
        self._c = C.c_void_p()
        a = np.array([[(x0 >> (64 * j)) & (2**64 - 1) for j in range(4)]], dtype=np.uint64)
        b = np.array([[(x1 >> (64 * j)) & (2**64 - 1) for j in range(4)]], dtype=np.uint64)
        fn = self.L.zl_circuit_poseidon_chain_witness if witness_only else self.L.zl_circuit_poseidon_chain
        rc = fn(curve, k, _p64(a), _p64(b), C.byref(self._c))
        if rc:
            raise BackendError(rc, "zl_circuit_poseidon_chain")
        self._export()

    def _export(self):
        self._view = R1csC()
        zp = u64p()
        self.L.zl_circuit_export(self._c, C.byref(self._view), C.byref(zp))
        self._zp = zp

    @classmethod
    def merkle(cls, curve: int, depth: int, leaf: int, index: int, path, witness_only: bool = False) -> "Circuit":
        """the Merkle-membership circuit (zl_circuit_poseidon_merkle): the fold of path (depth integers, bottom up) over leaf at position index equals the
        public root.  witness_only: as in the constructor."""
        self = cls.__new__(cls)
        self.L = load_library()
        self.curve = curve
        self.witness_only = witness_only
        self._c = C.c_void_p()
        words = lambda v: [(int(v) >> (64 * j)) & (2**64 - 1) for j in range(4)]
        lf = np.array([words(leaf)], dtype=np.uint64)
        pa = np.array([words(v) for v in path], dtype=np.uint64).reshape(-1, 4)
        if pa.shape[0] != depth or not 0 <= index < 2**64:
            raise BackendError(-1, "zl_circuit_poseidon_merkle")
        fn = self.L.zl_circuit_poseidon_merkle_witness if witness_only else self.L.zl_circuit_poseidon_merkle
        rc = fn(curve, depth, _p64(lf), index, _ptr_or_none(pa), C.byref(self._c))
        if rc:
            raise BackendError(rc, "zl_circuit_poseidon_merkle")
        self._export()
        return self

    @classmethod
    def _arity(cls, curve: int, inputs, depth: int, index: int, path, witness_only: bool, what: str) -> "Circuit":
        self = cls.__new__(cls)
        self.L = load_library()
        self.curve = curve
        self.witness_only = witness_only
        self._c = C.c_void_p()
        words = lambda v: [(int(v) >> (64 * j)) & (2**64 - 1) for j in range(4)]
        x = np.array([words(v) for v in inputs], dtype=np.uint64).reshape(-1, 4)
        arity = x.shape[0]
        if any(not 0 <= int(v) < 2**256 for v in list(inputs) + list(path)) or not 0 <= index < 2**64:
            raise BackendError(-1, what)
        if depth is None:
            fn = self.L.zl_circuit_poseidon_hash_witness if witness_only else self.L.zl_circuit_poseidon_hash
            rc = fn(curve, arity, _ptr_or_none(x), C.byref(self._c))
        else:
            pa = np.array([words(v) for v in path], dtype=np.uint64).reshape(-1, 4)
            if pa.shape[0] != depth:
                raise BackendError(-1, what)
            fn = self.L.zl_circuit_poseidon_merkle_leaf_witness if witness_only else self.L.zl_circuit_poseidon_merkle_leaf
            rc = fn(curve, arity, depth, _ptr_or_none(x), index, _ptr_or_none(pa), C.byref(self._c))
        if rc:
            raise BackendError(rc, what)
        self._export()
        return self

    @classmethod
    def poseidon_hash(cls, curve: int, inputs, witness_only: bool = False) -> "Circuit":
        """the hash circuit (zl_circuit_poseidon_hash): the Poseidon hash of `inputs` (2..5 integers: the arity) equals the public digest.  At arity 2 it is
        Circuit(curve, 1, inputs[0], inputs[1]).  witness_only: as in the constructor."""
        return cls._arity(curve, inputs, None, 0, [], witness_only, "zl_circuit_poseidon_hash")

    @classmethod
    def merkle_leaf(cls, curve: int, depth: int, preimage, index: int, path, witness_only: bool = False) -> "Circuit":
        """the leaf-membership circuit (zl_circuit_poseidon_merkle_leaf): the fold of path (depth integers, bottom up) over the Poseidon hash of `preimage`
        (2..5 integers: the arity) at position index equals the public root.  witness_only: as in the constructor."""
        return cls._arity(curve, preimage, depth, index, path, witness_only, "zl_circuit_poseidon_merkle_leaf")

    @classmethod
    def poseidon_encrypt(cls, curve: int, initial_state, key, header, plaintext, witness_only: bool = False) -> "Circuit":
        """the duplex-encryption circuit (zl_circuit_poseidon_encrypt): the public tag and ciphertext are the encryption of the secret `plaintext` -- N blocks of
        W - 1 integers each, which fixes the width W -- under the secret `key` (>= 1 integers) and the public `header`; initial_state: W integers or None (zero).
        Public inputs: tag, ciphertext, header.  witness_only: as in the constructor."""
        what = "zl_circuit_poseidon_encrypt"
        self = cls.__new__(cls)
        self.L = load_library()
        self.curve = curve
        self.witness_only = witness_only
        self._c = C.c_void_p()
        blocks = [list(b) for b in plaintext]
        width = len(blocks[0]) + 1 if blocks else 0
        flat = [v for b in blocks for v in b]
        st = None if initial_state is None else list(initial_state)
        if any(len(b) != width - 1 for b in blocks) or (st is not None and len(st) != width) or any(
                not 0 <= int(v) < 2**256 for v in flat + list(key) + list(header) + (st or [])):
            raise BackendError(-1, what)
        arr = lambda vs: np.array([[(int(v) >> (64 * j)) & (2**64 - 1) for j in range(4)] for v in vs], dtype=np.uint64).reshape(-1, 4)
        k, h, p, s0 = arr(key), arr(header), arr(flat), arr(st or [])
        fn = self.L.zl_circuit_poseidon_encrypt_witness if witness_only else self.L.zl_circuit_poseidon_encrypt
        rc = fn(curve, width, None if st is None else _p64(s0), _ptr_or_none(k), k.shape[0], _ptr_or_none(h), h.shape[0], _ptr_or_none(p), len(blocks),
                C.byref(self._c))
        if rc:
            raise BackendError(rc, what)
        self._export()
        return self

    @classmethod
    def hybrid_encrypt(cls, curve: int, initial_state, generator, esk: int, pk, header, plaintext, bits: Optional[int] = None, witness_only: bool = False) -> "Circuit":
        """the hybrid-encryption circuit (zl_circuit_hybrid_encrypt): the public (epk, tag, ciphertext) is the hybrid encryption, to the public key `pk` (x, y) over
        the public `generator` (x, y), of the secret `plaintext` -- N blocks of W - 1 integers each, which fixes the width W -- under the secret ephemeral key
        `esk` (below the subgroup order and below 2^bits; bits None: the full width) and the public `header`; initial_state: W integers or None (zero).  Public
        inputs: G, pk, epk, tag, ciphertext, header.  witness_only: as in the constructor."""
        what = "zl_circuit_hybrid_encrypt"
        self = cls.__new__(cls)
        self.L = load_library()
        self.curve = curve
        self.witness_only = witness_only
        self._c = C.c_void_p()
        bits = ed_order_bits(curve) if bits is None else bits
        blocks = [list(b) for b in plaintext]
        width = len(blocks[0]) + 1 if blocks else 0
        flat = [v for b in blocks for v in b]
        st = None if initial_state is None else list(initial_state)
        pts = [int(generator[0]), int(generator[1]), int(pk[0]), int(pk[1]), int(esk)]
        if any(len(b) != width - 1 for b in blocks) or (st is not None and len(st) != width) or not 0 <= bits < 2**32 or any(
                not 0 <= int(v) < 2**256 for v in flat + list(header) + (st or []) + pts):
            raise BackendError(-1, what)
        arr = lambda vs: np.array([[(int(v) >> (64 * j)) & (2**64 - 1) for j in range(4)] for v in vs], dtype=np.uint64).reshape(-1, 4)
        w, h, p, s0 = arr(pts), arr(header), arr(flat), arr(st or [])
        fn = self.L.zl_circuit_hybrid_encrypt_witness if witness_only else self.L.zl_circuit_hybrid_encrypt
        rc = fn(curve, width, bits, None if st is None else _p64(s0), _p64(w[:2]), _p64(w[4]), _p64(w[2:4]), _ptr_or_none(h), h.shape[0], _ptr_or_none(p), len(blocks),
                C.byref(self._c))
        if rc:
            raise BackendError(rc, what)
        self._export()
        return self

    @classmethod
    def ed_scalar_mul(cls, curve: int, point, scalar: int, bits: Optional[int] = None, witness_only: bool = False) -> "Circuit":
        """the scalar-multiplication circuit (zl_circuit_ed_scalar_mul): the public point Q is `scalar` times the public `point` (x, y) of the embedded curve, for a
        secret scalar below the subgroup order and below 2^bits; bits None: the full width of the curve.  Public inputs: P.x, P.y, Q.x, Q.y.  witness_only: as
        in the constructor."""
        what = "zl_circuit_ed_scalar_mul"
        self = cls.__new__(cls)
        self.L = load_library()
        self.curve = curve
        self.witness_only = witness_only
        self._c = C.c_void_p()
        bits = ed_order_bits(curve) if bits is None else bits
        vals = [int(point[0]), int(point[1]), int(scalar)]
        if any(not 0 <= v < 2**256 for v in vals) or not 0 <= bits < 2**32:
            raise BackendError(-1, what)
        w = np.array([[(v >> (64 * j)) & (2**64 - 1) for j in range(4)] for v in vals], dtype=np.uint64)
        fn = self.L.zl_circuit_ed_scalar_mul_witness if witness_only else self.L.zl_circuit_ed_scalar_mul
        rc = fn(curve, bits, _p64(w[:2]), _p64(w[2]), C.byref(self._c))
        if rc:
            raise BackendError(rc, what)
        self._export()
        return self

    def witness_only_compatible(self) -> bool:
        """a full compiler folded constants the way a witness-only run of the same circuit will (R1CS::witness_only_compatible)"""
        return self.L.zl_circuit_witness_only_compatible(self._c) == 1

    @property
    def shape(self):
        return self._view.n_constraints, self._view.n_instance, self._view.n_witness

    def is_satisfied(self) -> bool:
        return self.L.zl_circuit_is_satisfied(self._c) == 1

    def arrays(self) -> dict:
        """copy the CSR view + assignment into numpy (same dict layout Backend.groth16_prove takes)"""
        v = self._view
        out = {"n_constraints": v.n_constraints, "n_instance": v.n_instance, "n_witness": v.n_witness}
        for m, key in enumerate("ABC"):
            ptr = np.ctypeslib.as_array(v.row_ptr[m], shape=(v.n_constraints + 1,)).copy()
            nnz = int(ptr[-1])
            if nnz == 0:  # (a witness-only circuit exports no rows)
                col, val = np.zeros(0, dtype=np.uint32), np.zeros((0, 4), dtype=np.uint64)
            else:
                col = np.ctypeslib.as_array(v.col[m], shape=(nnz,)).copy()
                val = np.ctypeslib.as_array(v.val[m], shape=(nnz * 4,)).copy().reshape(nnz, 4)
            out[key] = (ptr, col, val)
        nv = v.n_instance + v.n_witness
        out["assignment"] = np.ctypeslib.as_array(self._zp, shape=(nv * 4,)).copy().reshape(nv, 4)
        return out

    def close(self):
        if self._c:
            self.L.zl_circuit_free(self._c)
            self._c = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Groth16Keys:
    """Groth16<E>::compile result (ProvingContext on the device), or -- from_bytes -- a ProvingContext decoded from its wire format."""

    def __init__(self, backend: Backend, circuit: Circuit, seed: int, _encoded: bytes = None, _flags: int = 0):
        self.L = backend.L
        self.backend = backend
        self.circuit = circuit
        self._k = C.c_void_p()
        if _encoded is None:
            backend._check(self.L.zl_groth16_compile(backend._ctx, circuit._c, seed, C.byref(self._k)), "zl_groth16_compile")
        else:
            buf = (C.c_uint8 * max(1, len(_encoded))).from_buffer_copy(_encoded if _encoded else b"\0")
            backend._check(self.L.zl_groth16_keys_from_bytes(backend._ctx, circuit.curve, buf, len(_encoded), _flags, C.byref(self._k)),
                           "zl_groth16_keys_from_bytes")
        self.pk = G16PkC()
        self.L.zl_groth16_keys_pk(self._k, C.byref(self.pk))
        n_c, n_i, n_w = circuit.shape
        nv = n_i + n_w
        log_n = max(1, (n_c + n_i - 1).bit_length())
        for name, cnt, grp in (("a_query", nv, ZL_G1), ("b_g1_query", nv, ZL_G1), ("h_query", (1 << log_n) - 1, ZL_G1), ("l_query", n_w, ZL_G1),
                               ("b_g2_query", nv, ZL_G2)):
            backend._bases[getattr(self.pk, name)] = (circuit.curve, grp, cnt)  # so Backend.bases_download works on them

    @classmethod
    def from_bytes(cls, backend: Backend, circuit: Circuit, data: bytes, check: bool = False) -> "Groth16Keys":
        """codec::Decode for ProvingContext (zl_groth16_keys_from_bytes); `circuit` is the circuit the key belongs to (proofs need it)"""
        return cls(backend, circuit, 0, _encoded=data, _flags=ZL_CHECK if check else 0)

    def _bytes_of(self, fn, what: str) -> bytes:
        n = C.c_size_t(0)
        self.backend._check(fn(self._k, None, 0, C.byref(n)), what)
        out = (C.c_uint8 * max(1, n.value))()
        self.backend._check(fn(self._k, out, n.value, C.byref(n)), what)
        return C.string_at(C.addressof(out), n.value)

    def to_bytes(self) -> bytes:
        """codec::Encode for ProvingContext: ark_groth16::ProvingKey serialize_unchecked (uncompressed)"""
        return self._bytes_of(self.L.zl_groth16_keys_to_bytes, "zl_groth16_keys_to_bytes")

    def vk_to_bytes(self) -> bytes:
        """ark_groth16::VerifyingKey serialize (compressed)"""
        return self._bytes_of(self.L.zl_groth16_vk_to_bytes, "zl_groth16_vk_to_bytes")

    def trapdoor(self):
        out = np.zeros((5, 4), dtype=np.uint64)
        self.backend._check(self.L.zl_groth16_keys_trapdoor(self._k, _p64(out)), "zl_groth16_keys_trapdoor")
        return [sum(int(v) << (64 * j) for j, v in enumerate(row)) for row in out]

    def pk_dict(self) -> dict:
        nq = FQ_LIMBS[self.circuit.curve]
        d = {k: getattr(self.pk, k) for k in ("a_query", "b_g1_query", "h_query", "l_query", "b_g2_query")}
        for k, n in (("alpha_g1", 2 * nq), ("beta_g1", 2 * nq), ("delta_g1", 2 * nq), ("beta_g2", 4 * nq), ("delta_g2", 4 * nq)):
            d[k] = np.ctypeslib.as_array(getattr(self.pk, k), shape=(n,)).copy()
        return d

    def prove(self, seed: int, circuit: Optional["Circuit"] = None, lane: Optional[Backend] = None):
        """Groth16::prove(context, compiler, rng=SplitMix64(seed)) -> ((a, a_inf, b, b_inf, c, c_inf), r, s); circuit: another compiler of the SAME circuit
        (e.g. a witness-only one with a new witness) instead of the one the keys were built with; lane: a fork() of the keys' backend to run on (one
        per host thread: concurrent proofs over one device-resident key)"""
        proof = G16ProofC()
        r = np.zeros(4, dtype=np.uint64)
        s = np.zeros(4, dtype=np.uint64)
        self.backend._check(self.L.zl_groth16_prove_circuit((lane or self.backend)._ctx, self._k, (circuit or self.circuit)._c, seed, C.byref(proof), _p64(r), _p64(s)),
                            "zl_groth16_prove_circuit")
        nq = FQ_LIMBS[self.circuit.curve]
        return (np.array(proof.a[: 2 * nq], dtype=np.uint64), proof.a_inf, np.array(proof.b[: 4 * nq], dtype=np.uint64), proof.b_inf,
                np.array(proof.c[: 2 * nq], dtype=np.uint64), proof.c_inf), r, s

    def prove_batch(self, assignments: np.ndarray, r: np.ndarray, s: np.ndarray, flags: int = 0, lane: Optional[Backend] = None):
        """zl_groth16_prove_batch over this key: assignments (count, n_variables, 4) of the keys' circuit, blinding scalars r, s (count, 4) -> `count` proofs.
        The circuit's matrices are uploaded to the keys' backend on first use (lanes read them there)."""
        if not getattr(self, "_r1cs", 0):
            self._r1cs = self.backend.r1cs_upload(self.circuit.curve, self.circuit.arrays())
        return (lane or self.backend)._prove_batch(self.pk, self.circuit.curve, self._r1cs, assignments, r, s, flags)

    def prove_batch_dev(self, d_assignments: int, count: int, r: np.ndarray, s: np.ndarray, flags: int = 0, lane: Optional[Backend] = None):
        """prove_batch over `count` dense assignments at the device address d_assignments (zl_groth16_prove_batch_dev)"""
        if not getattr(self, "_r1cs", 0):
            self._r1cs = self.backend.r1cs_upload(self.circuit.curve, self.circuit.arrays())
        return (lane or self.backend)._prove_batch_dev(self.pk, self.circuit.curve, self._r1cs, d_assignments, count, r, s, flags)

    def chain_links(self) -> int:
        """k when the keys' circuit has the shape of a k-link Poseidon chain, else 0"""
        n_c, n_i, n_w = self.circuit.shape
        k = (n_w - 2) // 234
        return k if k >= 1 and (n_c, n_i, n_w) == (234 * k + 1, 2, 2 + 234 * k) else 0

    def prove_chains(self, x0, x1, r: np.ndarray, s: np.ndarray, lane: Optional[Backend] = None):
        """zl_groth16_prove_poseidon_chains over this key: chain inputs x0, x1 and blinding scalars r, s (count, 4) -> (proofs, public inputs (count, 4));
        proof j is prove_batch's for the assignment of Circuit(curve, k, x0[j], x1[j]).  Keys of a circuit that is no Poseidon chain are refused."""
        k = self.chain_links()
        if not k:
            raise ValueError("prove_chains: the keys' circuit is not a Poseidon chain")
        if not getattr(self, "_r1cs", 0):
            self._r1cs = self.backend.r1cs_upload(self.circuit.curve, self.circuit.arrays())
        return (lane or self.backend)._prove_chains(self.pk, self.circuit.curve, self._r1cs, k, x0, x1, r, s)

    def merkle_depth(self) -> int:
        """d when the keys' circuit has the shape of a depth-d Merkle-membership circuit (Circuit.merkle), else 0"""
        n_c, n_i, n_w = self.circuit.shape
        d = (n_w - 1) // 238
        return d if 1 <= d <= 40 and (n_c, n_i, n_w) == (237 * d + 1, 2, 1 + 238 * d) else 0

    def _merkle_ready(self, what: str) -> int:
        d = self.merkle_depth()
        if not d:
            raise ValueError(what + ": the keys' circuit is not a Merkle-membership circuit")
        if not getattr(self, "_r1cs", 0):
            self._r1cs = self.backend.r1cs_upload(self.circuit.curve, self.circuit.arrays())
        return d

    def prove_merkle_paths(self, leaves, indices, paths, r: np.ndarray, s: np.ndarray, lane: Optional[Backend] = None):
        """zl_groth16_prove_merkle_paths over this key: leaves (count, 4), indices (count,), paths (count, depth, 4) and blinding scalars r, s (count, 4) ->
        (proofs, roots (count, 4)); proof j is prove_batch's for the assignment of Circuit.merkle(curve, depth, leaves[j], indices[j], paths[j]).  Keys of a
        circuit that is no membership circuit are refused."""
        d = self._merkle_ready("prove_merkle_paths")
        return (lane or self.backend)._prove_merkle_paths(self.pk, self.circuit.curve, self._r1cs, d, leaves, indices, paths, r, s)

    def prove_merkle_members(self, d_nodes: int, n: int, indices, r: np.ndarray, s: np.ndarray, lane: Optional[Backend] = None):
        """zl_groth16_prove_merkle_members over this key: the tree of n leaves at the device address d_nodes (Backend.poseidon_merkle_build_dev with the keys'
        depth) and leaf indices (count,) -> (proofs, the root (4,)): from tree to proofs with nothing but the indices going up"""
        d = self._merkle_ready("prove_merkle_members")
        return (lane or self.backend)._prove_merkle_members(self.pk, self.circuit.curve, self._r1cs, d_nodes, n, d, indices, r, s)

    def prove_forest_members(self, forest: "MerkleForest", tree_of, indices, r: np.ndarray, s: np.ndarray, lane: Optional[Backend] = None):
        """zl_groth16_prove_forest_members over this key: proof j shows that leaf indices[j] of tree tree_of[j] of the device forest (of the keys' depth) is in that
        tree -> (proofs, roots (count, 4): each proof's public input); byte for byte prove_merkle_members on forest.tree_nodes(tree_of[j]) with n = the capacity"""
        self._merkle_ready("prove_forest_members")
        return (lane or self.backend)._prove_forest_members(self.pk, self.circuit.curve, self._r1cs, forest, tree_of, indices, r, s)

    def hash_arity(self) -> int:
        """a when the keys' circuit has the shape of an arity-a hash circuit (Circuit.poseidon_hash), else 0; arity 2 is also the one-link chain"""
        n_c, n_i, n_w = self.circuit.shape
        for a, s3 in _ARITY_RECORDS.items():
            if (n_c, n_i, n_w) == (s3 + 1, 2, a + s3):
                return a
        return 0

    def merkle_leaf_shape(self):
        """(a, d) when the keys' circuit has the shape of a leaf-membership circuit of arity a and depth d (Circuit.merkle_leaf), else None"""
        n_c, n_i, n_w = self.circuit.shape
        d = n_w - n_c - 1
        for a, s3 in _ARITY_RECORDS.items():
            dd = d - (a - 2)
            if 1 <= dd <= 40 and (n_c, n_i, n_w) == (s3 + 237 * dd + 1, 2, a + s3 + 238 * dd):
                return a, dd
        return None

    def _upload_r1cs(self):
        if not getattr(self, "_r1cs", 0):
            self._r1cs = self.backend.r1cs_upload(self.circuit.curve, self.circuit.arrays())

    def prove_hashes(self, inputs, r: np.ndarray, s: np.ndarray, lane: Optional[Backend] = None):
        """zl_groth16_prove_poseidon_hashes over this key: inputs (count, arity, 4) and blinding scalars r, s (count, 4) -> (proofs, digests (count, 4));
        proof j is prove_batch's for the assignment of Circuit.poseidon_hash(curve, inputs[j]).  Keys of a circuit that is no hash circuit are refused."""
        a = self.hash_arity()
        if not a:
            raise ValueError("prove_hashes: the keys' circuit is not a Poseidon hash circuit")
        self._upload_r1cs()
        return (lane or self.backend)._prove_hashes(self.pk, self.circuit.curve, self._r1cs, a, inputs, r, s)

    def prove_encryptions(self, initial_state, keys, headers, plaintexts, r: np.ndarray, s: np.ndarray, lane: Optional[Backend] = None):
        """zl_groth16_prove_poseidon_encryptions over this key: operands as Backend.poseidon_duplex_encrypt and blinding scalars r, s (count, 4) -> (proofs, tags
        (count, 4), ciphertexts (count, N, W - 1, 4)); proof j is prove_batch's for the assignment of Circuit.poseidon_encrypt(curve, initial_state, keys[j],
        headers[j], plaintexts[j]).  Keys of a circuit that has not the shape of the operands' (W, K, H, N) are refused by the library (ZL_EINVAL)."""
        self._upload_r1cs()
        return (lane or self.backend)._prove_encryptions(self.pk, self.circuit.curve, self._r1cs, initial_state, keys, headers, plaintexts, r, s)

    def prove_hybrid_encryptions(self, initial_state, generator, esk, pks, headers, plaintexts, r: np.ndarray, s: np.ndarray, bits: Optional[int] = None,
                                 lane: Optional[Backend] = None):
        """zl_groth16_prove_hybrid_encryptions over this key: operands as Backend.hybrid_encrypt and blinding scalars r, s (count, 4) -> (proofs, epks (count, 2, 4),
        tags (count, 4), ciphertexts (count, N, W - 1, 4)); proof j is prove_batch's for the assignment of Circuit.hybrid_encrypt(curve, initial_state, generator,
        esk[j], pks[j], headers[j], plaintexts[j], bits).  bits None: the full width.  Keys of a circuit of another shape are refused by the library (ZL_EINVAL)."""
        self._upload_r1cs()
        bits = ed_order_bits(self.circuit.curve) if bits is None else bits
        return (lane or self.backend)._prove_hybrid_encryptions(self.pk, self.circuit.curve, self._r1cs, bits, initial_state, generator, esk, pks, headers, plaintexts, r, s)

    def prove_scalar_muls(self, points, scalars, r: np.ndarray, s: np.ndarray, bits: Optional[int] = None, lane: Optional[Backend] = None):
        """zl_groth16_prove_ed_scalar_muls over this key: points (count, 2, 4) or one point (2, 4), scalars (count, 4) and blinding scalars r, s (count, 4) ->
        (proofs, Q (count, 2, 4)); proof j is prove_batch's for the assignment of Circuit.ed_scalar_mul(curve, points[j], scalars[j], bits).  bits None: the
        full width.  Keys of a circuit of another `bits` are refused by the library (ZL_EINVAL)."""
        self._upload_r1cs()
        bits = ed_order_bits(self.circuit.curve) if bits is None else bits
        return (lane or self.backend)._prove_scalar_muls(self.pk, self.circuit.curve, self._r1cs, bits, points, scalars, r, s)

    def _leaf_ready(self, what: str):
        shape = self.merkle_leaf_shape()
        if shape is None:
            raise ValueError(what + ": the keys' circuit is not a leaf-membership circuit")
        self._upload_r1cs()
        return shape

    def prove_merkle_leaf_paths(self, preimages, indices, paths, r: np.ndarray, s: np.ndarray, lane: Optional[Backend] = None):
        """zl_groth16_prove_merkle_leaf_paths over this key: preimages (count, arity, 4), indices (count,), paths (count, depth, 4) and blinding scalars ->
        (proofs, roots (count, 4)); proof j is prove_batch's for the assignment of Circuit.merkle_leaf(curve, depth, preimages[j], indices[j], paths[j])"""
        a, d = self._leaf_ready("prove_merkle_leaf_paths")
        return (lane or self.backend)._prove_merkle_leaf_paths(self.pk, self.circuit.curve, self._r1cs, a, d, preimages, indices, paths, r, s)

    def prove_merkle_leaf_members(self, d_nodes: int, d_preimages: int, n: int, indices, r: np.ndarray, s: np.ndarray, lane: Optional[Backend] = None):
        """zl_groth16_prove_merkle_leaf_members over this key: the tree of n leaves at the device address d_nodes (of the keys' depth), the n x arity preimages
        of its leaves at d_preimages and leaf indices (count,) -> (proofs, the root (4,))"""
        a, d = self._leaf_ready("prove_merkle_leaf_members")
        return (lane or self.backend)._prove_merkle_leaf_members(self.pk, self.circuit.curve, self._r1cs, a, d_nodes, d_preimages, n, d, indices, r, s)

    def prove_many(self, seeds, circuits=None):
        """zl_groth16_prove_circuits: a stream of proofs over this key on two prover lanes (two host threads inside the library); proofs[i] is what
        prove(seeds[i], circuits[i]) returns.  circuits: None (the keys' own compiler for every proof) or one compiler per seed."""
        n = len(seeds)
        circuits = list(circuits) if circuits is not None else [self.circuit] * n
        assert len(circuits) == n
        cs = (C.c_void_p * max(1, n))(*[c._c for c in circuits])
        sd = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64))
        out = (G16ProofC * max(1, n))()
        self.backend._check(self.L.zl_groth16_prove_circuits(self.backend._ctx, self._k, cs, _p64(sd), n, out), "zl_groth16_prove_circuits")
        nq = FQ_LIMBS[self.circuit.curve]
        return [(np.array(p.a[: 2 * nq], dtype=np.uint64), p.a_inf, np.array(p.b[: 4 * nq], dtype=np.uint64), p.b_inf, np.array(p.c[: 2 * nq], dtype=np.uint64), p.c_inf)
                for p in out[:n]]

    def verify(self, proof, public_inputs: np.ndarray) -> bool:
        """Groth16::verify(vk, input, proof) with the host pairing; proof = (a, a_inf, b, b_inf, c, c_inf); public_inputs: (n_public, 4) canonical words
        (each < r; otherwise ZL_EINVAL, nothing computed, outputs untouched): a BackendError, not a verdict"""
        pc = _proof_struct(proof)
        pub = np.ascontiguousarray(public_inputs, dtype=np.uint64).reshape(-1, 4)
        ok = C.c_int(0)
        self.backend._check(self.L.zl_groth16_verify(self._k, _p64(pub), pub.shape[0], C.byref(pc), C.byref(ok)), "zl_groth16_verify")
        return bool(ok.value)

    def verify_batch(self, proofs, public_inputs, seed: Optional[int] = None, each: bool = False):
        """Groth16::verify of many proofs in one random linear combination (zl_groth16_verify_batch): device Miller loops and MSM, one host final
        exponentiation.  public_inputs: (count, n_public, 4) canonical words (each < r; otherwise ZL_EINVAL, nothing computed, outputs untouched: a
        BackendError for the whole batch, not a verdict), or anything that reshapes to it; seed=None draws the combination from the OS (what a verifier
        must do); an int makes it reproducible (tests).  Returns ok, or (ok, per-proof verdicts) with each=True."""
        n = len(proofs)
        pub_arr = np.asarray(public_inputs, dtype=np.uint64)
        if pub_arr.ndim == 3:
            n_public = pub_arr.shape[1]
        elif n:
            n_public = pub_arr.size // (4 * n)
        else:
            n_public = self.circuit.shape[1] - 1
        arr = _proofs_array(proofs)
        pub = _pubs_of(pub_arr, n, n_public)
        sd = np.array([seed or 0], dtype=np.uint64)
        ok = C.c_int(0)
        ev = np.zeros(max(1, n), dtype=np.uint8)
        self.backend._check(self.L.zl_groth16_verify_batch(self.backend._ctx, self._k, _p64(pub), n_public, arr, n, _p64(sd) if seed is not None else None,
                                                           C.byref(ok), ev.ctypes.data_as(u8p) if each else None), "zl_groth16_verify_batch")
        return (bool(ok.value), ev[:n].astype(bool)) if each else bool(ok.value)

    def verify_batch_bytes(self, data, count: int, public_inputs, seed: Optional[int] = None, each: bool = False, n_public: Optional[int] = None):
        """zl_groth16_verify_batch_bytes: verify_batch over `count` WIRE proofs (packed proof_to_bytes records): decoded on the device, then the random linear
        combination over the records that decoded.  public_inputs / seed as verify_batch: canonical (each < r; otherwise ZL_EINVAL, nothing computed, outputs
        untouched), those of a record that does not decode included; n_public overrides what the shape of public_inputs implies.
        Returns ok, or (ok, per-record verdicts, decode statuses (count,) int32) with each=True; a record that does not decode is a rejected proof."""
        pub_arr = np.asarray(public_inputs, dtype=np.uint64)
        if n_public is None:
            n_public = pub_arr.shape[1] if pub_arr.ndim == 3 else (pub_arr.size // (4 * count) if count else self.circuit.shape[1] - 1)
        buf = _bytes_view(data, 0, count * self.L.zl_groth16_proof_bytes(self.circuit.curve))
        pub = np.ascontiguousarray(pub_arr.reshape(-1))
        if not pub.size:
            pub = np.zeros(4, dtype=np.uint64)
        sd = np.array([seed or 0], dtype=np.uint64)
        ok = C.c_int(0)
        ev = np.zeros(max(1, count), dtype=np.uint8)
        st = np.zeros(max(1, count), dtype=np.int32)
        self.backend._check(self.L.zl_groth16_verify_batch_bytes(self.backend._ctx, self._k, _p64(pub), n_public, _addr(buf, 0), count, _p64(sd) if seed is not None else None,
                                                                 C.byref(ok), ev.ctypes.data_as(u8p) if each else None, st.ctypes.data_as(i32p) if each else None),
                            "zl_groth16_verify_batch_bytes")
        return (bool(ok.value), ev[:count].astype(bool), st[:count]) if each else bool(ok.value)

    def close(self):
        if getattr(self, "_r1cs", 0):
            self.backend.r1cs_free(self._r1cs)
            self._r1cs = 0
        if self._k:
            self.L.zl_groth16_keys_free(self._k)
            self._k = C.c_void_p()

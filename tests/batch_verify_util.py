"""Shared inputs of the batched-verification tests: oracle-made Groth16 proofs under a fixed trapdoor (Poseidon chain and the generic R1CS shapes of
r1cs_gen.py), the verifying key as canonical points, and the tampering cases every batch verifier must reject."""
import numpy as np

import groth16_util as gu
import oracle_lib as ol
import r1cs_gen as rg
from oracle_lib import po

TD = po.Groth16Trapdoor(alpha=0x1357_9BDF_2468, beta=0x0F0E_0D0C_0B0A, gamma=0x2222_3333_4444, delta=0x5A5A_A5A5_7777, tau=0x0123_4567_89AB_CDEF)


def circuit(curve, kind: str):
    """(cs, arrays) of the Poseidon chain (kind 'poseidon', one hash) or a generic shape of r1cs_gen.SHAPES"""
    if kind == "poseidon":
        cs = po.poseidon_chain_circuit(curve.fr, 1)
        return cs, gu.r1cs_arrays(cs)
    return rg.shape_case(curve, kind)


class Case:
    """a circuit, its oracle proving key under TD, and a verifying key as canonical points"""

    def __init__(self, curve, kind: str):
        self.curve = curve
        self.cs, self.arrays = circuit(curve, kind)
        self.pk = gu.setup_with_trapdoor(curve, self.cs, TD)
        self.z = ol.ints_to_limbs(self.cs.assignment(), 4)
        self.n_public = int(self.arrays["n_instance"]) - 1
        self.vk = {"alpha_g1": self.pk["alpha_g1"], "beta_g2": self.pk["beta_g2"], "gamma_g2": gu.g2_mul_gen(curve, [TD.gamma])[0],
                   "delta_g2": self.pk["delta_g2"], "gamma_abc": ol.oracle_g1_mul_gen(curve, ol.ints_to_limbs(self.pk["ex"]["gamma_abc"], 4))}

    def proofs(self, count: int, seed: int = 1):
        rs = ol.random_scalars(self.curve, 2 * count, seed)
        return [gu.oracle_prove(self.curve, self.arrays, self.z, self.pk, rs[2 * i], rs[2 * i + 1], threads=8)[0] for i in range(count)]

    def pubs(self, count: int) -> np.ndarray:
        """(count, n_public, 4): every proof proves the same statement"""
        return np.tile(self.z[1:1 + self.n_public][None], (count, 1, 1)).astype(np.uint64)

    def py_verify(self, proof, pub) -> bool:
        """per-proof verdict of the definition-level Python pairing (po.groth16_verify_pairing); A or B at infinity is invalid"""
        a, ai, b, bi, c, ci = proof
        if ai or bi:
            return False
        c_ = self.curve
        nq = ol.nlq(c_)
        g1 = lambda row: ol.limbs_to_point(c_, row, int(not np.asarray(row).any()))

        def g2(row):
            if not np.asarray(row).any():
                return None
            v = ol.limbs_to_ints(np.asarray(row).reshape(4, nq))
            return ((v[0], v[1]), (v[2], v[3]))

        vk = {"alpha_g1": g1(self.vk["alpha_g1"]), "beta_g2": g2(self.vk["beta_g2"]), "gamma_g2": g2(self.vk["gamma_g2"]),
              "delta_g2": g2(self.vk["delta_g2"]), "gamma_abc_g1": [g1(r) for r in self.vk["gamma_abc"]]}
        return po.groth16_verify_pairing(c_, vk, ol.limbs_to_ints(np.asarray(pub).reshape(-1, 4)), g1(a), g2(b), g1(c if not ci else np.zeros_like(c)))


def neg_g2(curve, b: np.ndarray) -> np.ndarray:
    """-B: (x, -y) on the twist"""
    nq = ol.nlq(curve)
    v = ol.limbs_to_ints(np.asarray(b).reshape(4, nq))
    p = curve.fq.p
    return ol.ints_to_limbs([v[0], v[1], (p - v[2]) % p, (p - v[3]) % p], nq).reshape(-1)


def tampered(curve, proofs, pubs, how: str):
    """(proofs, pubs, tampered indices) for one of the rejection cases; index 1 (and 2 for the swap) are changed"""
    proofs = [tuple(np.array(x, copy=True) if isinstance(x, np.ndarray) else x for x in p) for p in proofs]
    pubs = np.array(pubs, copy=True)
    if how == "public":
        pubs[1, 0, 0] ^= np.uint64(1)
        return proofs, pubs, {1}
    if how == "swap_c":
        p1, p2 = list(proofs[1]), list(proofs[2])
        p1[4], p2[4] = proofs[2][4].copy(), proofs[1][4].copy()
        proofs[1], proofs[2] = tuple(p1), tuple(p2)
        return proofs, pubs, {1, 2}
    if how == "neg_b":
        p1 = list(proofs[1])
        p1[2] = neg_g2(curve, p1[2])
        proofs[1] = tuple(p1)
        return proofs, pubs, {1}
    if how == "a_inf":
        p1 = list(proofs[1])
        p1[0] = np.zeros_like(p1[0])
        p1[1] = 1
        proofs[1] = tuple(p1)
        return proofs, pubs, {1}
    if how in ("b_inf", "c_inf"):  # the point as a decoder hands over infinity: all-zero words and the flag
        p1 = list(proofs[1])
        at = 2 if how == "b_inf" else 4
        p1[at] = np.zeros_like(p1[at])
        p1[at + 1] = 1
        proofs[1] = tuple(p1)
        return proofs, pubs, {1}
    if how == "offcurve_b":
        p1 = list(proofs[1])
        b = p1[2].copy()
        b[0] ^= np.uint64(1)  # x.c0 + / - 1: not a point of the twist any more (coordinates stay canonical)
        p1[2] = b
        proofs[1] = tuple(p1)
        return proofs, pubs, {1}
    raise ValueError(how)


TAMPER_CASES = ["public", "swap_c", "neg_b", "a_inf"]
INF_CASES = ["b_inf", "c_inf"]  # B at infinity is invalid by rule, C at infinity by the pairing equation

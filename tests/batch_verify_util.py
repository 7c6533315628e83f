"""Shared inputs of the batched-verification tests: oracle-made Groth16 proofs under a fixed trapdoor (Poseidon chain and the generic R1CS shapes of
r1cs_gen.py), the verifying key as canonical points, and the tampering cases every batch verifier must reject."""
import ctypes as C
import os

import numpy as np

import groth16_util as gu
import oracle_lib as ol
import r1cs_gen as rg
from oracle_lib import po
from openzl_amd.backend import _addr, _bytes_view, _p64, _proof_struct, _proofs_array, _pubs_of, i32p, load_library, u8p

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
    if how == "public_alias":  # x + r: the same residue in other words.  Not a verdict: every verifier refuses the call (ZL_EINVAL), so not in TAMPER_CASES
        pubs = with_publics(pubs, {(1, 0): aliases(curve, ol.limbs_to_ints(pubs[1, 0])[0])[0]})
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


# ---- public inputs that are not canonical ---------------------------------------------------------------------------------------------------------------
def aliases(curve, x: int):
    """every x + k r, k >= 1, that fits four u64 words: other encodings of the residue x.  x < r gives k = 1..4 and 5 where it fits on BN254
    (2^256 = 5.29 r), k = 1 and 2 where it fits on BLS12-381 (2^256 = 2.21 r); never empty"""
    r = curve.fr.p
    assert 0 <= x < r
    return list(range(x + r, 1 << 256, r))


def with_publics(pubs, plan: dict) -> np.ndarray:
    """a copy of pubs (count, n_public, 4) with the integer plan[(proof, position)] written as four words at that place"""
    pubs = np.array(pubs, copy=True)
    for (i, j), v in plan.items():
        pubs[i, j] = ol.ints_to_limbs([v], 4)[0]
    return pubs


def public_ints(case: "Case") -> list:
    """the public inputs of the statement every proof of a case proves"""
    return ol.limbs_to_ints(case.pubs(1)[0])


def wide_public_plans(case: "Case", count: int) -> list:
    """[(label, {(proof, position): value})]: the batches of `count` proofs in which a public input is not below r.  Every alias of the true value at
    the first and the last position of the first, the middle and the last proof; two proofs at once; r where the value is 0 and 2r - 1 where it is r - 1
    (statements that hold them: "many_publics"); 2^256 - 1 and 2^255, which are wide and alias nothing in particular."""
    r, x, last = case.curve.fr.p, public_ints(case), case.n_public - 1
    where = sorted({0, count // 2, count - 1})
    plans = [(f"proof {i} public {j} + {k} r", {(i, j): v}) for j in sorted({0, last}) for i in where for k, v in enumerate(aliases(case.curve, x[j]), 1)]
    if count > 1:
        plans.append(("two proofs", {(0, 0): aliases(case.curve, x[0])[0], (count - 1, last): aliases(case.curve, x[last])[-1]}))
    if 0 in x:
        plans.append(("r for 0", {(count // 2, x.index(0)): r}))
    if r - 1 in x:
        plans.append(("2r - 1 for r - 1", {(count // 2, x.index(r - 1)): 2 * r - 1}))
    plans.append(("2^256 - 1", {(count // 2, last): (1 << 256) - 1}))
    plans.append(("2^255", {(0, 0): 1 << 255}))
    return plans


def with_vars(names: dict, fn):
    """fn() with the environment variables of `names` set (the ZL_TUNE_* knobs are read on every call), restored afterwards"""
    old = {k: os.environ.get(k) for k in names}
    try:
        for k, v in names.items():
            os.environ[k] = str(v)
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---- the verifying entry points as C calls over pre-filled outputs: what a refusal must leave as the caller set it ---------------------------------------
OK_SENTINEL, EACH_SENTINEL, STATUS_SENTINEL = 0x5AFE5AFE, 0xA5, 0x7A7A7A7A


class Outputs:
    """the return code of one verifying call and what *ok, ok_each and status (bytes-in verifier only) hold after it"""

    def __init__(self, n: int, status: bool = False):
        self.n = n
        self.rc = None
        self._ok = C.c_int(OK_SENTINEL)
        self._each = np.full(max(1, n), EACH_SENTINEL, dtype=np.uint8)
        self._status = np.full(max(1, n), STATUS_SENTINEL, dtype=np.int32) if status else None

    @property
    def untouched(self) -> bool:
        return (self._ok.value == OK_SENTINEL and bool((self._each == EACH_SENTINEL).all())
                and (self._status is None or bool((self._status == STATUS_SENTINEL).all())))

    @property
    def ok(self) -> bool:
        assert self.rc == 0 and self._ok.value in (0, 1)
        return bool(self._ok.value)

    @property
    def each(self) -> list:
        assert self.rc == 0 and set(self._each[:self.n].tolist()) <= {0, 1}
        return [bool(e) for e in self._each[:self.n]]

    @property
    def status(self) -> list:
        assert self.rc == 0
        return self._status[:self.n].tolist()


def _flat_pubs(pubs) -> np.ndarray:
    pub = np.ascontiguousarray(np.asarray(pubs, dtype=np.uint64).reshape(-1))
    return pub if pub.size else np.zeros(4, dtype=np.uint64)


def _seed(seed):
    return _p64(np.array([seed], dtype=np.uint64)) if seed is not None else None


def call_host(case: Case, proofs, pubs, seed=5) -> Outputs:
    """zl_test_verify_batch_host over the verifying key of `case`: no ctx, all on the host"""
    out = Outputs(len(proofs))
    vk = [np.ascontiguousarray(case.vk[k], dtype=np.uint64) for k in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc")]
    out.rc = load_library().zl_test_verify_batch_host(case.curve.cid, *[_p64(v) for v in vk], case.n_public, _proofs_array(proofs), _p64(_flat_pubs(pubs)),
                                                      len(proofs), _seed(seed), C.byref(out._ok), out._each.ctypes.data_as(u8p))
    return out


def call_verify(k, proof, pub) -> Outputs:
    """zl_groth16_verify of one proof under the key handle k"""
    out = Outputs(0)
    pub = np.ascontiguousarray(pub, dtype=np.uint64).reshape(-1, 4)
    pc = _proof_struct(proof)
    out.rc = load_library().zl_groth16_verify(k, _p64(_flat_pubs(pub)), pub.shape[0], C.byref(pc), C.byref(out._ok))
    return out


def call_batch(backend, k, proofs, pubs, n_public: int, seed=5) -> Outputs:
    """zl_groth16_verify_batch under the key handle k"""
    out = Outputs(len(proofs))
    out.rc = backend.L.zl_groth16_verify_batch(backend._ctx, k, _p64(_flat_pubs(pubs)), n_public, _proofs_array(proofs), len(proofs), _seed(seed),
                                               C.byref(out._ok), out._each.ctypes.data_as(u8p))
    return out


def call_batch_bytes(backend, k, curve, data: bytes, count: int, pubs, n_public: int, seed=5) -> Outputs:
    """zl_groth16_verify_batch_bytes over `count` packed wire proofs under the key handle k"""
    out = Outputs(count, status=True)
    buf = _bytes_view(data, 0, count * backend.L.zl_groth16_proof_bytes(curve.cid))
    out.rc = backend.L.zl_groth16_verify_batch_bytes(backend._ctx, k, _p64(_flat_pubs(pubs)), n_public, _addr(buf, 0), count, _seed(seed), C.byref(out._ok),
                                                     out._each.ctypes.data_as(u8p), out._status.ctypes.data_as(i32p))
    return out


def verify_raw(backend, k, proofs, pubs, n_public: int, seed):
    """(ok, per-proof verdicts) of zl_groth16_verify_batch under the key handle k; an error code raises BackendError"""
    _pubs_of(pubs, len(proofs), n_public)  # the shape
    out = call_batch(backend, k, proofs, pubs, n_public, seed)
    backend._check(out.rc, "zl_groth16_verify_batch")
    return out.ok, np.array(out.each, dtype=bool)


# ---- the oracle's key of a Case as the backend's key object ----------------------------------------------------------------------------------------------
def _g1_pts(curve, arr):
    arr = np.asarray(arr).reshape(-1, 2 * ol.nlq(curve))
    return [ol.limbs_to_point(curve, row, int(not row.any())) for row in arr]


def _g2_pts(curve, arr):
    nq = ol.nlq(curve)
    out = []
    for row in np.asarray(arr).reshape(-1, 4 * nq):
        v = ol.limbs_to_ints(row.reshape(4, nq))
        out.append(None if not row.any() else ((v[0], v[1]), (v[2], v[3])))
    return out


def oracle_pk_bytes(case: Case) -> bytes:
    """the oracle's proving key of a case in the wire format, encoded by the Python restatement"""
    c = case.curve
    pk = case.pk
    vk = {"alpha_g1": _g1_pts(c, pk["alpha_g1"])[0], "beta_g2": _g2_pts(c, pk["beta_g2"])[0], "gamma_g2": _g2_pts(c, case.vk["gamma_g2"])[0],
          "delta_g2": _g2_pts(c, pk["delta_g2"])[0], "gamma_abc_g1": _g1_pts(c, case.vk["gamma_abc"])}
    pts = {"vk": vk, "beta_g1": _g1_pts(c, pk["beta_g1"])[0], "delta_g1": _g1_pts(c, pk["delta_g1"])[0], "a_query": _g1_pts(c, pk["a_query"]),
           "b_g1_query": _g1_pts(c, pk["b_g1_query"]), "b_g2_query": _g2_pts(c, pk["b_g2_query"]), "h_query": _g1_pts(c, pk["h_query"]),
           "l_query": _g1_pts(c, pk["l_query"])}
    return po.groth16_pk_bytes(c, pts)


def oracle_keys(backend, case: Case):
    """the key handle of oracle_pk_bytes decoded by zl_groth16_keys_from_bytes; the caller frees it (zl_groth16_keys_free)"""
    data = oracle_pk_bytes(case)
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    k = C.c_void_p()
    backend._check(backend.L.zl_groth16_keys_from_bytes(backend._ctx, case.curve.cid, buf, len(data), 0, C.byref(k)), "zl_groth16_keys_from_bytes")
    return k

"""The public inputs of a Groth16 verifier are canonical words, each below r; device half.  The batches of tests/test_verify_public_input_contract_cpu.py
(batch_verify_util.wide_public_plans: every alias x + k r at the first and the last position of the first, the middle and the last proof, two proofs at once,
r for 0, 2r - 1 for r - 1, 2^256 - 1, 2^255) through every verifying entry point: zl_groth16_verify, zl_groth16_verify_batch under the key of a Groth16Keys
object and under a bare key handle, zl_groth16_verify_batch_bytes, and the host hook beside them.  Each refuses with ZL_EINVAL, leaves *ok, ok_each and
status as the caller set them, and the same ctx then gives the canonical batch its ordinary verdict: in a valid batch, a batch of one, a rejected batch whose
per-proof products run as device final exponentiations, on host threads and over several launch sets, and the bytes-in verifier whether or not the record
beside the wide word decodes.  Canonical 0, 1, r - 2 and r - 1 keep their ordinary verdicts on every entry."""
import numpy as np
import pytest

import batch_verify_util as bv
from oracle_lib import po
from openzl_amd import Groth16Keys
from openzl_amd.backend import BackendError, proof_from_bytes, proof_to_bytes

pytestmark = pytest.mark.gpu

CURVES = [po.BLS12_381, po.BN254]
KINDS = ["many_publics", "poseidon"]  # 39 public inputs with 0, 1 and r - 1 among them; one public input
COUNT = 5
HOST_ONLY = 1 << 30  # a chunk never holds that many proofs: the host threads
KNOBS = [{"ZL_TUNE_FEXP_DEV_MIN": 1, "ZL_TUNE_FEXP_CHUNK": 3}, {"ZL_TUNE_FEXP_DEV_MIN": HOST_ONLY}, {"ZL_TUNE_PAIR_SET": 4}]


class _CircuitShape:
    """what a Groth16Keys object reads of its circuit when it only verifies: the oracle's circuits have no compiler object on this side"""

    def __init__(self, case):
        self.curve = case.curve.cid
        self.shape = tuple(int(case.arrays[k]) for k in ("n_constraints", "n_instance", "n_witness"))


class _Dev:
    """a case with its oracle key twice on the device: inside a Groth16Keys object (keys) and as a bare handle (rawk)"""

    def __init__(self, backend, curve, kind):
        self.backend, self.curve = backend, curve
        self.case = bv.Case(curve, kind)
        self.n_public = self.case.n_public
        self.proofs = self.case.proofs(COUNT, seed=5)
        self.keys = Groth16Keys.from_bytes(backend, _CircuitShape(self.case), bv.oracle_pk_bytes(self.case))
        self.rawk = bv.oracle_keys(backend, self.case)

    def close(self):
        self.backend.L.zl_groth16_keys_free(self.rawk)
        self.keys.close()

    def wire(self, proofs) -> bytes:
        return b"".join(proof_to_bytes(self.curve.cid, p) for p in proofs)

    def calls(self, proofs, pubs, data=None) -> dict:
        """name -> Outputs of every batch entry point over one batch (data: the wire records when they are not simply the proofs')"""
        n, be = len(proofs), self.backend
        return {"host hook": bv.call_host(self.case, proofs, pubs),
                "verify_batch, Groth16Keys' key": bv.call_batch(be, self.keys._k, proofs, pubs, self.n_public),
                "verify_batch, bare key handle": bv.call_batch(be, self.rawk, proofs, pubs, self.n_public),
                "verify_batch_bytes": bv.call_batch_bytes(be, self.keys._k, self.curve, data or self.wire(proofs), n, pubs, self.n_public)}

    def refused(self, proofs, pubs, plan, label, data=None):
        """every entry point refuses the batch `pubs`, whose wide words sit at the places of `plan`, and writes nothing"""
        outs = self.calls(proofs, pubs, data)
        for i in sorted({i for i, _ in plan}):
            outs[f"verify, proof {i}"] = bv.call_verify(self.keys._k, proofs[i], pubs[i])
        for name, out in outs.items():
            assert out.rc == -1, f"{label}, {name}: a public input at or above r must be refused with ZL_EINVAL, the call returned {out.rc}"
            assert out.untouched, f"{label}, {name}: a refused call wrote to its outputs"
        i = min(i for i, _ in plan)
        for call in (lambda: self.keys.verify(proofs[i], pubs[i]), lambda: self.keys.verify_batch(proofs, pubs, seed=5, each=True),
                     lambda: self.keys.verify_batch_bytes(data or self.wire(proofs), len(proofs), pubs, seed=5, each=True)):
            with pytest.raises(BackendError) as e:
                call()
            assert e.value.code == -1, label

    def verdicts(self, proofs, pubs, expected, label):
        """every entry point gives the canonical batch `pubs` the per-proof verdicts `expected`"""
        for name, out in self.calls(proofs, pubs).items():
            assert out.rc == 0 and out.ok == all(expected) and out.each == expected, f"{label}, {name}"
            assert name != "verify_batch_bytes" or not any(out.status)
        assert [self.keys.verify(p, x) for p, x in zip(proofs, pubs)] == expected, label
        ok, each = self.keys.verify_batch(proofs, pubs, seed=5, each=True)
        assert ok == all(expected) and each.tolist() == expected, label
        ok, each, st = self.keys.verify_batch_bytes(self.wire(proofs), len(proofs), pubs, seed=5, each=True)
        assert ok == all(expected) and each.tolist() == expected and not st.any(), label

    def every_plan_refused(self, proofs, pubs, expected, label):
        """each wide batch made from the canonical batch (proofs, pubs) is refused; after each refusal the same ctx gives the canonical batch its
        verdicts `expected`, and at the end every entry point does"""
        n = len(proofs)
        for what, plan in bv.wide_public_plans(self.case, n):
            self.refused(proofs, bv.with_publics(pubs, plan), plan, f"{label}, {what}")
            out = bv.call_batch(self.backend, self.keys._k, proofs, pubs, self.n_public)
            assert out.rc == 0 and out.ok == all(expected) and out.each == expected, f"{label}, after {what}"
        self.verdicts(proofs, pubs, expected, label)


@pytest.fixture(scope="module", params=[(c, k) for c in CURVES for k in KINDS], ids=lambda p: f"{p[0].name}-{p[1]}")
def dev(request, backend):
    d = _Dev(backend, *request.param)
    yield d
    d.close()


def test_wide_public_input_is_refused_in_an_otherwise_valid_batch(dev):
    dev.every_plan_refused(dev.proofs, dev.case.pubs(COUNT), [True] * COUNT, "valid batch")


def test_wide_public_input_is_refused_in_a_batch_of_one(dev):
    dev.every_plan_refused(dev.proofs[:1], dev.case.pubs(1), [True], "batch of one")


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: ",".join(f"{n[8:]}={v}" for n, v in k.items()))
def test_wide_public_input_is_refused_where_the_per_proof_products_would_read_it(dev, knobs):
    """proof 1 has -B: the combination fails and the per-proof products run over every proof, the one with the wide word among them -- as device final
    exponentiations three to a launch, on host threads, and one proof per launch set"""
    bad, pubs, idx = bv.tampered(dev.curve, dev.proofs, dev.case.pubs(COUNT), "neg_b")
    assert all(not {i for i, _ in plan} & idx for _, plan in bv.wide_public_plans(dev.case, COUNT))
    expected = [i not in idx for i in range(COUNT)]
    bv.with_vars(knobs, lambda: dev.every_plan_refused(bad, pubs, expected, f"rejected batch under {knobs}"))


def test_public_alias_tamper_case_is_refused(dev):
    bad, pubs, idx = bv.tampered(dev.curve, dev.proofs[:3], dev.case.pubs(3), "public_alias")
    dev.refused(bad, pubs, {(i, 0): None for i in idx}, "public_alias")


def test_bytes_in_verifier_refuses_whether_or_not_the_record_decodes(dev):
    """the wide word belongs to record 2; in the second half one byte of that record's A is broken so that it does not decode.  All count x n_public words
    are checked ahead of the decoder: the refusal is the same, and so is the canonical batch's verdict afterwards (that record marked, with its status)"""
    cid, pubs = dev.curve.cid, dev.case.pubs(COUNT)
    recs = [proof_to_bytes(cid, p) for p in dev.proofs]
    broken = None
    for at in range(len(recs[2]) // 4):  # A is the first quarter of a record (A, then B at twice its size, then C)
        cand = recs[2][:at] + bytes([recs[2][at] ^ 1]) + recs[2][at + 1:]
        try:
            proof_from_bytes(cid, cand)
        except BackendError:
            broken = recs[:2] + [cand] + recs[3:]
            break
    assert broken is not None, "no single-bit change of A that the host decoder refuses"
    plans = [(what, plan) for what, plan in bv.wide_public_plans(dev.case, COUNT) if {i for i, _ in plan} == {2}]
    assert plans
    for data, expected in ((b"".join(recs), [True] * COUNT), (b"".join(broken), [i != 2 for i in range(COUNT)])):
        for what, plan in plans:
            out = bv.call_batch_bytes(dev.backend, dev.keys._k, dev.curve, data, COUNT, bv.with_publics(pubs, plan), dev.n_public)
            assert out.rc == -1 and out.untouched, what
            with pytest.raises(BackendError) as e:
                dev.keys.verify_batch_bytes(data, COUNT, bv.with_publics(pubs, plan), seed=5, each=True)
            assert e.value.code == -1, what
        out = bv.call_batch_bytes(dev.backend, dev.keys._k, dev.curve, data, COUNT, pubs, dev.n_public)
        assert out.rc == 0 and out.ok == all(expected) and out.each == expected and [s == 0 for s in out.status] == expected


def test_an_empty_batch_is_accepted_whatever_the_words(dev):
    wide = np.full((1, max(1, dev.n_public), 4), (1 << 64) - 1, dtype=np.uint64)
    for out in (bv.call_host(dev.case, [], wide), bv.call_batch(dev.backend, dev.keys._k, [], wide, dev.n_public),
                bv.call_batch(dev.backend, dev.rawk, [], wide, dev.n_public),
                bv.call_batch_bytes(dev.backend, dev.keys._k, dev.curve, b"", 0, wide, dev.n_public)):
        assert out.rc == 0 and out.ok and out.each == []


@pytest.mark.parametrize("old,new", [(None, None), (-1, -2), (0, 1)], ids=["unchanged", "r-1_to_r-2", "0_to_1"])
def test_canonical_boundary_values_get_an_ordinary_verdict(dev, old, new):
    """the statement with 0, 1 and r - 1 among its public inputs is accepted; r - 2 for r - 1 or 1 for 0 in proof 1 is another statement in canonical
    words: rejected with exactly that proof marked, not an error"""
    r, x, pubs, expected = dev.curve.fr.p, bv.public_ints(dev.case), dev.case.pubs(3), [True] * 3
    if old is not None:
        at = x.index(old % r) if dev.n_public > 1 else 0  # the statement with one public input: its neighbour below / above
        pubs = bv.with_publics(pubs, {(1, at): (x[at] + new - old) % r})
        expected[1] = False
    dev.verdicts(dev.proofs[:3], pubs, expected, f"{old} -> {new}")

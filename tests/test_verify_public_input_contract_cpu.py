"""The public inputs of a Groth16 verifier are canonical words, each below r; host half (no GPU): zl_test_verify_batch_host, the NULL-ctx path of the batch
verifier.  x + k r is the residue x, so a verifier that reduces the words (or walks all their bits over a point of order r) takes x and x + k r as one
statement, while a caller that keys on the 32 bytes it handed over sees two.  The entry point must refuse such a call -- ZL_EINVAL, *ok and ok_each left as
the caller set them -- wherever the word sits and whichever path would have read it: the accepted combination, the per-proof products of a rejected batch, a
batch of one.  The canonical neighbours (0, 1, r - 2, r - 1) keep their ordinary verdicts, which equal the definition-level Python pairing."""
import pytest

import batch_verify_util as bv
import oracle_lib as ol
from oracle_lib import po
from openzl_amd.backend import BackendError, hook_verify_batch_host

CURVES = [po.BLS12_381, po.BN254]
KINDS = ["many_publics", "poseidon"]  # 39 public inputs with 0, 1 and r - 1 among them; one public input
COUNT = 5
_CASES = {}


def _case(curve, kind):
    key = (curve.cid, kind)
    if key not in _CASES:
        c = bv.Case(curve, kind)
        _CASES[key] = (c, c.proofs(COUNT, seed=5))
    return _CASES[key]


def _refused(case, proofs, pubs, label):
    out = bv.call_host(case, proofs, pubs)
    assert out.rc == -1, f"{label}: a public input at or above r must be refused with ZL_EINVAL, the call returned {out.rc}"
    assert out.untouched, f"{label}: a refused call wrote to *ok or ok_each"


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_aliases_are_every_other_encoding_of_the_residue(curve):
    r = curve.fr.p
    for x in (0, 1, 2, r // 2, (1 << 256) % r, (1 << 256) % r - 1, (1 << 256) % r + 1, r - 2, r - 1):
        al = bv.aliases(curve, x)
        assert al == [x + k * r for k in range(1, len(al) + 1)] and al[-1] < 1 << 256 <= al[-1] + r
        assert len(al) >= (4 if curve is po.BN254 else 1)
    # the last multiple fits for some residues only: both lengths occur
    assert {len(bv.aliases(curve, x)) for x in (0, r - 1)} == ({5, 4} if curve is po.BN254 else {2, 1})


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_many_publics_statement_holds_the_boundary_values(curve):
    case, _ = _case(curve, "many_publics")
    x = bv.public_ints(case)
    assert len(x) == case.n_public == 39 and {0, 1, curve.fr.p - 1} <= set(x)
    labels = [label for label, _ in bv.wide_public_plans(case, COUNT)]
    assert "r for 0" in labels and "2r - 1 for r - 1" in labels


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("kind", KINDS)
def test_wide_public_input_is_refused_in_an_otherwise_valid_batch(curve, kind):
    case, proofs = _case(curve, kind)
    for label, plan in bv.wide_public_plans(case, COUNT):
        _refused(case, proofs, bv.with_publics(case.pubs(COUNT), plan), label)
    for label, plan in bv.wide_public_plans(case, 1):
        _refused(case, proofs[:1], bv.with_publics(case.pubs(1), plan), "batch of one, " + label)
    out = bv.call_host(case, proofs, case.pubs(COUNT))
    assert out.rc == 0 and out.ok and all(out.each)


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("kind", KINDS)
def test_wide_public_input_is_refused_where_the_per_proof_products_would_read_it(curve, kind):
    """proof 1 has -B: the combination fails and verify_each runs over every proof, the one with the wide word among them"""
    case, proofs = _case(curve, kind)
    bad, pubs, idx = bv.tampered(curve, proofs, case.pubs(COUNT), "neg_b")
    for label, plan in bv.wide_public_plans(case, COUNT):
        assert not {i for i, _ in plan} & idx
        _refused(case, bad, bv.with_publics(pubs, plan), "rejected batch, " + label)
    out = bv.call_host(case, bad, pubs)
    assert out.rc == 0 and not out.ok and out.each == [i not in idx for i in range(COUNT)]


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_public_alias_tamper_case_is_a_refusal_not_a_verdict(curve):
    assert "public_alias" not in bv.TAMPER_CASES
    for kind in KINDS:
        case, proofs = _case(curve, kind)
        bad, pubs, idx = bv.tampered(curve, proofs[:3], case.pubs(3), "public_alias")
        assert idx == {1} and ol.limbs_to_ints(pubs[1, 0])[0] == bv.public_ints(case)[0] + curve.fr.p
        _refused(case, bad, pubs, "public_alias")
        with pytest.raises(BackendError) as e:
            hook_verify_batch_host(curve.cid, case.vk, bad, pubs, case.n_public, seed=5)
        assert e.value.code == -1


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_an_empty_batch_is_accepted_whatever_the_words(curve):
    case, _ = _case(curve, "many_publics")
    wide = bv.with_publics(case.pubs(1), {(0, 0): (1 << 256) - 1, (0, 38): curve.fr.p})
    out = bv.call_host(case, [], wide)
    assert out.rc == 0 and out.ok and out.each == []


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("old,new", [(-1, -2), (0, 1)], ids=["r-1_to_r-2", "0_to_1"])
def test_canonical_neighbours_get_an_ordinary_verdict(curve, old, new):
    """r - 2 for a public r - 1, 1 for a public 0: canonical words of another statement.  Rejected with exactly that proof marked, as the definition-level
    pairing says; not an error"""
    case, proofs = _case(curve, "many_publics")
    r, x, n = curve.fr.p, bv.public_ints(case), 3
    at = x.index(old % r)
    pubs = bv.with_publics(case.pubs(n), {(1, at): new % r})
    out = bv.call_host(case, proofs[:n], pubs)
    assert out.rc == 0 and not out.ok and out.each == [True, False, True]
    assert out.each == [case.py_verify(proofs[i], pubs[i]) for i in range(n)]

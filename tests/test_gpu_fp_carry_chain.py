"""The carry-chain field Fp<P> (openzl_amd/csrc/zl_field.h) and Fp2<P> over it on the device, on raw words: zl_test_fp_op against Python integers -- not
against the host hook -- for the four fields and the three multipliers: the out-of-line product scan (form 0), the inlined one that the Poseidon, NTT and G1
units compile (form 1) and the portable loop (form 2).  The cases are those of tests/test_fp_carry_chain_host.py (tests/fp_edge_util.py): operands where
carries, borrows and the final subtraction take their rare turns, and -- the multiplier's contract -- second operands and converted words at or above p.
Every case runs whole and at 1, 63, 64 and 65 records (a partial block, a full one, one lane into the next) with a sentinel row behind the output.

Then what follows from the contract: a point with a coordinate written x + k q is the same point to the device Miller loops, the batch verifier, the host
pairing and zl_bases_upload."""
import numpy as np
import pytest

import batch_verify_util as bv
import fp_edge_util as fe
import groth16_util as gu
import oracle_lib as ol
from oracle_lib import po
from openzl_amd import ZL_G1, ZL_G2, Groth16Keys
from openzl_amd.backend import ZL_CHECK, hook_fp_op, hook_pairing_product, hook_pairing_product_scaled

pytestmark = pytest.mark.gpu

FORMS = [0, 1, 2]
COUNTS = [1, 63, 64, 65]
CURVES = [po.BLS12_381, po.BN254]
SENTINEL = 0xA5C3F00D
HOST_ONLY = 1 << 30
KNOBS = [{"ZL_TUNE_FEXP_DEV_MIN": 1, "ZL_TUNE_FEXP_CHUNK": 3}, {"ZL_TUNE_FEXP_DEV_MIN": HOST_ONLY}, {"ZL_TUNE_PAIR_SET": 4}]  # as tests/test_gpu_verify_batch_reject.py
field_form = pytest.mark.parametrize("F,form", [(F, form) for F in fe.FIELDS for form in FORMS], ids=lambda v: str(v))


def _run_cases(backend, F, form, names):
    report = {}
    for name in names:
        op, rec, exp = fe.case_arrays(F, name)
        got = hook_fp_op(backend, F.fid, form, op, rec)
        bad = fe.wrong_rows(got, exp)
        if bad:
            report[name] = f"{bad} of {len(exp)} wrong"
        for n in COUNTS:
            if n > len(exp):
                continue
            out = np.full((n + 1, exp.shape[1]), SENTINEL, dtype=np.uint32)
            hook_fp_op(backend, F.fid, form, op, rec, n=n, out=out)
            if fe.wrong_rows(out[:n], exp[:n]) or not (out[n] == SENTINEL).all():
                report[f"{name}, {n} records"] = f"{fe.wrong_rows(out[:n], exp[:n])} of {n} wrong, sentinel {'kept' if (out[n] == SENTINEL).all() else 'OVERWRITTEN'}"
    assert not report, f"{F} form {form}: {report}"


@field_form
def test_canonical_operands_equal_python_integers(backend, F, form):
    _run_cases(backend, F, form, [n for n in fe.all_cases(F) if not fe.is_wide(n)])


@field_form
def test_values_at_or_above_p_are_read_as_their_residue(backend, F, form):
    _run_cases(backend, F, form, [n for n in fe.all_cases(F) if fe.is_wide(n)])


@field_form
def test_inverse_times_value_is_one(backend, F, form):
    op, rec, _ = fe.case_arrays(F, "inv")
    both = np.array(rec, copy=True)
    both[:, 1] = hook_fp_op(backend, F.fid, form, op, rec)
    prod = fe.ints(hook_fp_op(backend, F.fid, form, fe.MUL, both))
    assert prod == [F.R % F.p if v else 0 for v in fe.ints(rec[:, 0])]


# ---- consequences: a coordinate written x + k q ------------------------------------------------------------------------------------------------------------
_PTS = {}


def _points(curve):
    if curve.cid not in _PTS:
        ks = list(range(3, 67))
        _PTS[curve.cid] = (ol.oracle_g1_mul_gen(curve, ol.ints_to_limbs(ks, 4)), gu.g2_mul_gen(curve, ks))
    return _PTS[curve.cid]


def _ks(curve, row, coord):
    return sorted({1, fe.k_max(fe.fq_of(curve), fe.coord_int(curve, row, coord))})


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_pairing_products_of_a_rewritten_point_equal_the_canonical_ones(backend, curve):
    """two pairs; the G1 point of the first, then the G2 point of the second, carries x + k q.  Device Miller loops (zl_pairing_product), the production
    driver with and without scalars (zl_test_pairing_product_scaled) and the host lock-step loops all give the canonical pairs' value"""
    g1, g2 = _points(curve)
    i, ca, _ = fe.pick_lossy(curve, g1, [0, 1])
    j, cb, _ = fe.pick_lossy(curve, g2, [0, 1, 2, 3])
    ps, qs = np.stack([g1[i], g1[1]]), np.stack([g2[2], g2[j]])
    sc = np.array([[5, 0], [(1 << 64) - 3, 7]], dtype=np.uint64)
    want = hook_pairing_product(curve.cid, ps, qs)
    want_sc = hook_pairing_product_scaled(backend, curve.cid, ps, qs, sc)
    assert backend.pairing_product(curve.cid, ps, qs).tobytes() == want.tobytes()
    variants = [(np.stack([fe.rewrite_coord(curve, g1[i], ca, k), g1[1]]), qs) for k in _ks(curve, g1[i], ca)]
    variants += [(ps, np.stack([g2[2], fe.rewrite_coord(curve, g2[j], cb, k)])) for k in _ks(curve, g2[j], cb)]
    for p2, q2 in variants:
        assert hook_pairing_product(curve.cid, p2, q2).tobytes() == want.tobytes()
        assert backend.pairing_product(curve.cid, p2, q2).tobytes() == want.tobytes()
        assert hook_pairing_product_scaled(backend, curve.cid, p2, q2, None).tobytes() == want.tobytes()
        assert hook_pairing_product_scaled(backend, curve.cid, p2, q2, sc).tobytes() == want_sc.tobytes()


class _CircuitShape:
    """what a Groth16Keys object reads of its circuit when it only verifies"""

    def __init__(self, case):
        self.curve = case.curve.cid
        self.shape = tuple(int(case.arrays[k]) for k in ("n_constraints", "n_instance", "n_witness"))


@pytest.fixture(scope="module", params=CURVES, ids=lambda c: c.name)
def proved(request, backend):
    case = bv.Case(request.param, "poseidon")
    keys = Groth16Keys.from_bytes(backend, _CircuitShape(case), bv.oracle_pk_bytes(case))
    yield case, keys, case.proofs(12, seed=11)
    keys.close()


def test_a_valid_proof_with_a_rewritten_coordinate_stays_valid_on_every_path(proved):
    """A.x + k q (k = 1 and the largest that fits), and a coordinate of A, B and C at which the old host conversion lost a carry: zl_groth16_verify (host
    pairing) and zl_groth16_verify_batch accept it, alone and -- beside a proof with -B, so that the per-proof products run -- under every knob"""
    case, keys, proofs = proved
    curve = case.curve
    variants = [(fe.rewrite_coord(curve, proofs[0][0], 0, k),) + tuple(proofs[0][1:]) for k in _ks(curve, proofs[0][0], 0)]
    for at, coords in ((0, [0, 1]), (2, [0, 1, 2, 3]), (4, [0, 1])):
        i, coord, k = fe.pick_lossy(curve, [p[at] for p in proofs], coords)
        p = list(proofs[i])
        p[at] = fe.rewrite_coord(curve, p[at], coord, k)
        variants.append(tuple(p))
    pub1, pub3 = case.pubs(1), case.pubs(3)
    assert keys.verify(proofs[0], pub1[0]) is True
    for v in variants:
        assert keys.verify(v, pub1[0]) is True
        ok, each = keys.verify_batch([v], pub1, seed=7, each=True)
        assert ok is True and each.tolist() == [True]
        batch, _, idx = bv.tampered(curve, [v, proofs[1], proofs[2]], pub3, "neg_b")
        assert idx == {1}
        for knobs in KNOBS:
            ok, each = bv.with_vars(knobs, lambda: keys.verify_batch(batch, pub3, seed=7, each=True))
            assert ok is False and each.tolist() == [True, False, True], knobs


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("group", [ZL_G1, ZL_G2], ids=["g1", "g2"])
@pytest.mark.parametrize("flags", [0, ZL_CHECK], ids=["unchecked", "checked"])
def test_uploaded_bases_with_a_rewritten_coordinate_are_the_canonical_points(backend, curve, group, flags):
    """8 points, one coordinate of one of them written + k q: zl_bases_upload (with and without ZL_CHECK) stores the canonical point -- zl_bases_download
    returns the canonical words, and an 8-point MSM over the handle equals the MSM over the canonical upload"""
    g1, g2 = _points(curve)
    pts = np.ascontiguousarray((g1 if group == ZL_G1 else g2)[:8])
    s = ol.random_scalars(curve, 8, 77)
    h = backend.bases_upload(curve.cid, pts, group=group, flags=flags)
    want, want_inf = backend.msm(h, s)
    backend.bases_free(h)
    coord = 0 if group == ZL_G1 else 3
    for k in _ks(curve, pts[5], coord):
        alt = np.array(pts, copy=True)
        alt[5] = fe.rewrite_coord(curve, pts[5], coord, k)
        h = backend.bases_upload(curve.cid, alt, group=group, flags=flags)
        try:
            assert backend.bases_download(h).tobytes() == pts.tobytes(), k
            got, inf = backend.msm(h, s)
            assert inf == want_inf and got.tobytes() == want.tobytes(), k
        finally:
            backend.bases_free(h)

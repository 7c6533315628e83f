"""Compressed points and Groth16 proofs decoded on the device (zl_points_from_bytes_batch, zl_groth16_proofs_from_bytes_batch, zl_groth16_verify_batch_bytes;
csrc/zl_decode_dev.hip).  The expected value everywhere is the existing host decoder (zl_point_from_bytes / zl_groth16_proof_from_bytes, decode_util.py):
valid records at counts around the wave size, the whole record set shuffled so that failing and valid lanes share waves, the same set from an odd byte
offset, the Fq2 square root alone, real proofs with six tampered records through the decoder and the bytes-in batch verifier, and an MSM and a batch
verification on a ctx whose first call was a decode."""
import numpy as np
import pytest

import decode_util as du
import oracle_lib as ol
from oracle_lib import po
from openzl_amd import Backend, Circuit, Groth16Keys
from openzl_amd.backend import BackendError, hook_fq2_sqrt, proof_to_bytes

pytestmark = pytest.mark.gpu

CASES = [(c, g) for c in du.CURVES for g in (1, 2)]
IDS = [f"{c.name}-g{g}" for c, g in CASES]


def _same(got, exp, what):
    (xy, inf, st), (exy, einf, est) = got, exp
    bad = [i for i in range(len(est)) if st[i] != est[i] or inf[i] != einf[i] or (xy[i] != exy[i]).any()]
    assert not bad, (what, bad[:8], [int(st[i]) for i in bad[:8]], [int(est[i]) for i in bad[:8]])


@pytest.mark.parametrize("curve,group", CASES, ids=IDS)
def test_valid_points_at_counts_around_the_wave_size(backend, curve, group):
    recs = du.valid_records(curve, group)
    exy, einf, est = du.host_decode(curve, group, recs)
    assert not est.any() and not einf.any() and len(recs) >= 12
    for count in (0, 1, 63, 64, 65, 130):
        idx = np.arange(count) % len(recs)
        got = backend.points_from_bytes(curve.cid, group, b"".join(recs[i] for i in idx), count)
        assert got[0].shape == (count, exy.shape[1]) and got[1].shape == (count,) and got[2].shape == (count,)
        _same(got, (exy[idx], einf[idx], est[idx]), count)


@pytest.mark.parametrize("curve,group", CASES, ids=IDS)
def test_whole_record_set_shuffled_and_from_an_odd_offset(backend, curve, group):
    recs = du.records(curve, group)
    exy, einf, est = du.expected(curve, group)
    # two shuffles of the set behind each other: more than one wave, failing and valid lanes side by side in each
    rng = np.random.default_rng(40 + 2 * curve.cid + group)
    order = np.concatenate([rng.permutation(len(recs)), rng.permutation(len(recs))])
    assert len(order) > 64
    data = b"".join(recs[i][1] for i in order)
    exp = (exy[order], einf[order], est[order])
    _same(backend.points_from_bytes(curve.cid, group, data, len(order)), exp, "shuffled")
    buf = np.frombuffer(b"\xa5" + data + b"\x5a", dtype=np.uint8)  # the records start one byte into the buffer
    _same(backend.points_from_bytes(curve.cid, group, buf, len(order), offset=1), exp, "offset 1")


@pytest.mark.parametrize("curve", du.CURVES, ids=lambda c: c.name)
def test_fq2_sqrt_device(backend, curve):
    vals = du.sqrt_inputs(curve)
    roots, ok = hook_fq2_sqrt(backend, curve.cid, du.fq2_words(curve, vals))
    du.check_sqrt(curve, vals, roots, ok)
    hroots, hok = hook_fq2_sqrt(None, curve.cid, du.fq2_words(curve, vals))
    assert (ok == hok).all() and (roots == hroots).all()  # one template on both sides


N_PROOFS = 70
# record -> what was done to it (four do not decode, A at infinity decodes and is rejected by the verifier, the last is a sound proof of another statement)
TAMPERED = {3: "a_noncanonical", 17: "b_offcurve", 31: "b_nonsubgroup", 45: "c_no_y", 64: "a_infinity", 69: "other_public"}
DECODE_FAILS = {3: du.EINVAL, 17: du.ENOTCURVE, 31: du.ENOTCURVE, 45: du.ENOTCURVE}


@pytest.fixture(scope="module", params=du.CURVES, ids=lambda c: c.name)
def wire(request, backend):
    """70 proofs of the one-hash Poseidon circuit on the wire, six of them tampered, and their public inputs"""
    curve = request.param
    circ = Circuit(curve.cid, 1)
    keys = Groth16Keys(backend, circ, seed=0xDEC0DE)
    proofs = keys.prove_many(list(range(500, 500 + N_PROOFS)))
    pub = circ.arrays()["assignment"][1:2]
    pubs = np.tile(pub[None], (N_PROOFS, 1, 1)).astype(np.uint64)
    clean = [proof_to_bytes(curve.cid, p) for p in proofs]
    n1, n2 = du.nb(curve), 2 * du.nb(curve)
    recs = list(clean)
    for i, how in TAMPERED.items():
        a, b, c = recs[i][:n1], recs[i][n1:n1 + n2], recs[i][n1 + n2:]
        if how == "a_noncanonical":
            a = du.first(curve, 1, "x_eq_q")
        elif how == "b_offcurve":
            b = du.first(curve, 2, "no_y")
        elif how == "b_nonsubgroup":
            b = du.first(curve, 2, "outside_subgroup_large")
        elif how == "c_no_y":
            c = du.first(curve, 1, "no_y_big")
        elif how == "a_infinity":
            a = du.first(curve, 1, "infinity")
        else:
            pubs[i, 0, 0] ^= np.uint64(1)
        recs[i] = a + b + c
    yield curve, keys, clean, recs, pubs
    keys.close()


def test_proofs_decode_like_the_host_loop(backend, wire):
    curve, keys, clean, recs, pubs = wire
    tuples, st = backend.proofs_from_bytes(curve.cid, b"".join(recs), N_PROOFS)
    from openzl_amd.backend import _proof_struct

    for i, rec in enumerate(recs):
        est, epc = du.host_proof(curve, rec)
        assert st[i] == est == DECODE_FAILS.get(i, du.OK), (i, st[i], est)
        assert du.proof_fields(_proof_struct(tuples[i])) == du.proof_fields(epc), i
    none, st0 = backend.proofs_from_bytes(curve.cid, b"", 0)
    assert none == [] and st0.size == 0


def test_verify_batch_bytes(backend, wire):
    curve, keys, clean, recs, pubs = wire
    ok, each, st = keys.verify_batch_bytes(b"".join(recs), N_PROOFS, pubs, seed=5, each=True)
    assert ok is False
    assert [i for i in range(N_PROOFS) if not each[i]] == sorted(TAMPERED)
    assert {i: int(st[i]) for i in range(N_PROOFS) if st[i]} == DECODE_FAILS
    good = [i for i in range(N_PROOFS) if i not in TAMPERED]
    assert len(good) == 64
    ok, each, st = keys.verify_batch_bytes(b"".join(clean[i] for i in good), 64, pubs[good], seed=5, each=True)
    assert ok is True and each.all() and not st.any()
    assert keys.verify_batch_bytes(b"".join(clean[i] for i in good), 64, pubs[good]) is True  # seed from the OS, no per-record outputs
    assert keys.verify_batch_bytes(b"", 0, np.zeros((0, 1, 4), dtype=np.uint64)) is True
    with pytest.raises(BackendError) as e:
        keys.verify_batch_bytes(b"".join(clean[:2]), 2, np.zeros((2, 2, 4), dtype=np.uint64), seed=5)
    assert e.value.code == -1


def test_msm_and_verify_batch_after_a_decode_on_a_fresh_ctx(wire):
    """the decoder's slots beside the MSM's and the pairing product's (csrc/zl_ctx.h): a ctx whose first call is a decode then runs an ordinary MSM and a
    batch verification, and decodes again"""
    curve, keys, clean, recs, pubs = wire
    n = 1 << 10
    B = ol.oracle_g1_mul_gen(curve, ol.random_scalars(curve, n, 9101))
    S = ol.random_scalars(curve, n, 9102)
    exp = ol.oracle_msm_g1(curve, B, S, algo=0, threads=8)
    be = Backend(0)
    k2 = None
    try:
        first = be.proofs_from_bytes(curve.cid, b"".join(recs), N_PROOFS)
        h = be.bases_upload(curve.cid, B)
        xy, inf = be.msm(h, S)
        assert inf == exp[1] and (xy == exp[0]).all()
        k2 = Groth16Keys.from_bytes(be, keys.circuit, keys.to_bytes())
        good = [i for i in range(N_PROOFS) if i not in TAMPERED][:8]
        assert k2.verify_batch([first[0][i] for i in good], pubs[good], seed=2) is True
        assert k2.verify_batch_bytes(b"".join(recs[i] for i in good), 8, pubs[good], seed=2) is True
        again = be.proofs_from_bytes(curve.cid, b"".join(recs), N_PROOFS)
        assert (again[1] == first[1]).all() and all(np.array_equal(np.asarray(x), np.asarray(y)) for p, q in zip(again[0], first[0]) for x, y in zip(p, q))
    finally:
        if k2 is not None:
            k2.close()
        be.close()

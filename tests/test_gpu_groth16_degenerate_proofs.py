"""Groth16 provers on the blinding scalars of tests/groth16_degenerate_util.py: (r, s) chosen, through the known discrete logs of a trapdoor key, so that an
addition in a proof's tail meets equal operands (its doubling branch), opposite operands (the sum is infinity) or an operand at infinity, and so that A, B or
C themselves are the point at infinity.  Every case, on every path -- the resident prover with C from four MSMs and from the folded query, the batched prover
with host and with device assignments (A, B, C as multi-MSMs), the sharded prover over three virtual ranks -- must return the words and infinity flags the
exponents predict, byte for byte (tests/test_groth16_degenerate_cases_cpu.py pins those to the C oracle); each path then proves one ordinary random (r, s)
on the same ctx.  Then the range contract: every prover refuses an r or s at or above the modulus (ZL_EINVAL) and goes on working.  Shapes `smallest`
(N = 2) and `full16` (N = 16) on both curves; every comparison is exact."""
import numpy as np
import pytest

import groth16_degenerate_util as du
import groth16_util as gu
import oracle_lib as ol
from oracle_lib import po
from openzl_amd import BackendError, Circuit, Groth16Keys, MultiBackend
from test_gpu_groth16_generic import TD

pytestmark = pytest.mark.gpu
CURVES = [po.BLS12_381, po.BN254]
EINVAL = -1
EVERY = pytest.mark.parametrize("curve,shape", [(c, sh) for c in CURVES for sh in du.SHAPES], ids=lambda v: getattr(v, "name", v))
PARTS = ("a", "a_inf", "b", "b_inf", "c", "c_inf")


def dev(a: np.ndarray):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def resident(backend):
    """per (curve, shape): the trapdoor key and the matrices, uploaded once"""
    made = {}

    def get(curve, shape):
        key = (curve.cid, shape)
        if key not in made:
            cs, arrays, pk = du.shape_key(curve, shape, TD)
            made[key] = (gu.upload_pk(backend, curve, pk), backend.r1cs_upload(curve.cid, arrays))
        return made[key]

    yield get
    for dpk, hr in made.values():
        backend.r1cs_free(hr)
        gu.free_pk(backend, dpk)


@pytest.fixture
def device_path(monkeypatch):
    monkeypatch.setenv("ZL_TUNE_G16_BATCH_LOG_N", "28")
    monkeypatch.setenv("ZL_TUNE_G16_BATCH_MIN", "1")
    return monkeypatch


def _same(got, exp, label):
    for part, x, e in zip(PARTS, got, exp):
        assert np.array_equal(np.asarray(x), np.asarray(e)), (label, part)


def _ordinary(g, seed):
    """one random (r, s) and the oracle's proof of the group's assignment"""
    r, s = ol.random_scalars(g.curve, 2, seed)
    exp, _ = gu.oracle_prove(g.curve, g.arrays, g.zl, g.pk, r, s, threads=1)
    assert not (exp[1] or exp[3] or exp[5])
    return r, s, exp


def _rows(g, count):
    return np.ascontiguousarray(np.broadcast_to(g.zl, (count,) + g.zl.shape))


def _ran_on_device(backend):
    with pytest.raises(BackendError) as e:
        backend.groth16_last_h(2)  # a device batch leaves no single quotient
    assert e.value.code == EINVAL


@EVERY
@pytest.mark.parametrize("fold", ["0", "20"], ids=["four_msm", "folded"])
def test_resident_prover(backend, resident, monkeypatch, curve, shape, fold):
    """ZL_TUNE_G16_FOLD_LOG_N = 0: C from four MSMs (g16_run_g1_four); 20: the folded query (the c_fixed chain)"""
    monkeypatch.setenv("ZL_TUNE_G16_FOLD_LOG_N", fold)
    dpk, hr = resident(curve, shape)
    for which in du.ASSIGNMENTS:
        g = du.group(curve, shape, which, TD)
        cases, r, s, exp = g.rs_limbs()
        for j, c in enumerate(cases):
            _same(backend.groth16_prove_resident(curve.cid, dpk, hr, g.zl, r[j], s[j]), exp[j], (which, c.name, c.what))
        assert (backend.groth16_last_h(g.n) == g.h).all()
        ro, so, eo = _ordinary(g, 0xA0 + int(fold))
        _same(backend.groth16_prove_resident(curve.cid, dpk, hr, g.zl, ro, so), eo, (which, "ordinary"))


@EVERY
@pytest.mark.parametrize("where", ["host", "device"])
def test_batched_prover(backend, resident, device_path, curve, shape, where):
    """all cases of one assignment in one call, then A, B, C at infinity as calls of count 1: zl_groth16_prove_batch (host rows) and _batch_dev (device rows)"""
    dpk, hr = resident(curve, shape)

    def prove(g, r, s):
        count = r.shape[0]
        Z = _rows(g, count)
        if where == "host":
            got = backend.groth16_prove_batch(curve.cid, dpk, hr, Z, r, s)
        else:
            d_z = dev(Z)
            got = backend.groth16_prove_batch_dev(curve.cid, dpk, hr, d_z.data_ptr(), count, r, s)
        _ran_on_device(backend)
        assert len(got) == count
        return got

    for which in du.ASSIGNMENTS:
        g = du.group(curve, shape, which, TD)
        cases, r, s, exp = g.rs_limbs()
        for c, got, e in zip(cases, prove(g, r, s), exp):
            _same(got, e, (which, c.name, c.what))
        cases, r, s, exp = g.rs_limbs(du.IS_INFINITY)
        assert len(cases) == 3
        for j, c in enumerate(cases):
            _same(prove(g, r[j:j + 1], s[j:j + 1])[0], exp[j], (which, c.name, "alone"))
        ro, so, eo = _ordinary(g, 0xB0 + (where == "device"))
        _same(prove(g, ro.reshape(1, 4), so.reshape(1, 4))[0], eo, (which, "ordinary"))


@EVERY
def test_sharded_prover(curve, shape):
    """three virtual ranks; A / B / C at infinity and the doubling cases of A only: every proof uploads its key again"""
    mb = MultiBackend([0, 0, 0])
    try:
        for which in du.ASSIGNMENTS:
            g = du.group(curve, shape, which, TD)
            cases, r, s, exp = g.rs_limbs(du.SHARDED)
            assert len(cases) == len(du.SHARDED)
            for j, c in enumerate(cases):
                _same(mb.groth16_prove_sharded(curve.cid, g.pk, g.arrays, g.zl, r[j], s[j]), exp[j], (which, c.name, c.what))
            ro, so, eo = _ordinary(g, 0xC0)
            _same(mb.groth16_prove_sharded(curve.cid, g.pk, g.arrays, g.zl, ro, so), eo, (which, "ordinary"))
    finally:
        mb.close()


# ---- the range contract of r and s ------------------------------------------------------------------------------------------------------------------------
def _bad_values(curve):
    p = curve.fr.p
    return [p, p + 1, 1 << 255, (1 << 256) - 1]


def _refused(call):
    with pytest.raises(BackendError) as e:
        call()
    assert e.value.code == EINVAL


def _bad_pairs(curve, good):
    """(r, s) with one of them at or above the modulus and the other canonical"""
    for v in _bad_values(curve):
        bad = ol.ints_to_limbs([v], 4)[0]
        yield bad, good
        yield good, bad


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_single_provers_refuse_wide_blinding_scalars(backend, resident, curve):
    """zl_groth16_prove, _resident and _sharded: r or s = p, p + 1, 2^255, 2^256 - 1 is ZL_EINVAL; the next ordinary proof on the ctx equals the oracle's"""
    shape = "full16"
    dpk, hr = resident(curve, shape)
    g = du.group(curve, shape, "satisfying", TD)
    ro, so, eo = _ordinary(g, 0xD0)
    mb = MultiBackend([0, 0, 0])
    try:
        for r, s in _bad_pairs(curve, ro):
            _refused(lambda: backend.groth16_prove(curve.cid, dpk, g.arrays, g.zl, r, s))
            _refused(lambda: backend.groth16_prove_resident(curve.cid, dpk, hr, g.zl, r, s))
            _refused(lambda: mb.groth16_prove_sharded(curve.cid, g.pk, g.arrays, g.zl, r, s))
        _same(mb.groth16_prove_sharded(curve.cid, g.pk, g.arrays, g.zl, ro, so), eo, "sharded")
    finally:
        mb.close()
    _same(backend.groth16_prove(curve.cid, dpk, g.arrays, g.zl, ro, so), eo, "prove")
    _same(backend.groth16_prove_resident(curve.cid, dpk, hr, g.zl, ro, so), eo, "resident")


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("on_device", [True, False], ids=["device_path", "resident_loop"])
def test_batched_provers_refuse_wide_blinding_scalars(backend, resident, monkeypatch, curve, on_device):
    """zl_groth16_prove_batch with the bad value first, last and alone, and _batch_dev: the whole call is ZL_EINVAL on the device path and on the loop over
    the resident prover (the default bounds send five proofs there); the next ordinary batch equals the oracle's"""
    if on_device:
        monkeypatch.setenv("ZL_TUNE_G16_BATCH_LOG_N", "28")
        monkeypatch.setenv("ZL_TUNE_G16_BATCH_MIN", "1")
    else:
        monkeypatch.delenv("ZL_TUNE_G16_BATCH_LOG_N", raising=False)
        monkeypatch.delenv("ZL_TUNE_G16_BATCH_MIN", raising=False)
    shape = "full16"
    dpk, hr = resident(curve, shape)
    g = du.group(curve, shape, "satisfying", TD)
    count = 5
    good = ol.random_scalars(curve, 2 * count, 0xE0)
    Z = _rows(g, count)
    d_z = dev(Z)
    for v in _bad_values(curve):
        bad = ol.ints_to_limbs([v], 4)[0]
        for which in (0, 1):
            for at, n in ((0, count), (count - 1, count), (0, 1)):
                rs = [good[:n].copy(), good[count:count + n].copy()]
                rs[which][at] = bad
                _refused(lambda: backend.groth16_prove_batch(curve.cid, dpk, hr, Z[:n], rs[0], rs[1]))
                _refused(lambda: backend.groth16_prove_batch_dev(curve.cid, dpk, hr, d_z.data_ptr(), n, rs[0], rs[1]))
    exp = [gu.oracle_prove(curve, g.arrays, g.zl, g.pk, good[j], good[count + j], threads=1)[0] for j in range(count)]
    for got in (backend.groth16_prove_batch(curve.cid, dpk, hr, Z, good[:count], good[count:]),
                backend.groth16_prove_batch_dev(curve.cid, dpk, hr, d_z.data_ptr(), count, good[:count], good[count:])):
        if on_device:
            _ran_on_device(backend)
        for j in range(count):
            _same(got[j], exp[j], j)


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_fused_hash_prover_refuses_wide_blinding_scalars(backend, device_path, curve):
    """Groth16Keys.prove_hashes (arity 2), one of the provers that make their assignments on the device: the same refusal at index 0, last and alone, on
    the device path and on the loop over the resident prover; the next ordinary proofs equal the oracle's over the downloaded key"""
    xs = [[3, 1000], [5, 1007], [7, 1014]]
    count = len(xs)
    v = ol.ints_to_limbs([e for x in xs for e in x], 4).reshape(count, 2, 4)
    full = Circuit.poseidon_hash(curve.cid, xs[0])
    keys = Groth16Keys(backend, full, seed=0xF00D)
    try:
        good = ol.random_scalars(curve, 2 * count, 0xF0)
        for min_count in ("1", str(count + 1)):
            device_path.setenv("ZL_TUNE_G16_BATCH_MIN", min_count)
            for val in _bad_values(curve):
                bad = ol.ints_to_limbs([val], 4)[0]
                for which in (0, 1):
                    for at, n in ((0, count), (count - 1, count), (0, 1)):
                        rs = [good[:n].copy(), good[count:count + n].copy()]
                        rs[which][at] = bad
                        _refused(lambda: keys.prove_hashes(v[:n], rs[0], rs[1]))
        arrays = full.arrays()
        pk = keys.pk_dict()
        for name in ("a_query", "b_g1_query", "h_query", "l_query", "b_g2_query"):
            pk[name] = backend.bases_download(pk[name])
        exp, _ = gu.oracle_prove(curve, arrays, arrays["assignment"], pk, good[0], good[count], threads=8)
        for min_count in ("1", str(count + 1)):
            device_path.setenv("ZL_TUNE_G16_BATCH_MIN", min_count)
            got, pub = keys.prove_hashes(v, good[:count], good[count:])
            assert len(got) == count and np.array_equal(pub[0], arrays["assignment"][1])
            _same(got[0], exp, ("hashes", min_count))
    finally:
        keys.close()
        full.close()

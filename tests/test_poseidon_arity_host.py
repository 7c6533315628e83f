"""Poseidon at every arity of the specification table on the HOST (no device): zl_poseidon_spec, the generated constants against the oracle and the reference's
own numbers, the width-generic permutation against the Python model of tests/poseidon_arity_util.py -- itself pinned here to po.poseidon_permute -- and the
batched entry points with ctx == NULL."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle_lib as ol
import poseidon_arity_util as pa
import poseidon_util as pu
from oracle_lib import po
from openzl_amd import backend as zb
from openzl_amd import poseidon_constants, poseidon_permute, poseidon_spec

HERE = os.path.dirname(os.path.abspath(__file__))
FX = json.load(open(os.path.join(HERE, "golden", "ref_poseidon_fixtures.json")))
CURVES = pytest.mark.parametrize("curve", pa.CURVES, ids=lambda c: c.name)
WIDTHS = pytest.mark.parametrize("width", pa.WIDTHS)
ARITIES = pytest.mark.parametrize("arity", pa.ARITIES)
EINVAL = -1


def states3d(states):
    """a list of equal-width states -> (count, W, 4) words"""
    w = len(states[0])
    return pu.limbs([v for s in states for v in s]).reshape(len(states), w, 4)


# ---- the helper is pinned first ---------------------------------------------------------------------------------------------------------------------
@CURVES
@WIDTHS
def test_helper_equals_the_oracle_permutation(curve, width):
    rf, rp = pa.rounds(width)
    st = [curve.fr.p - 1, 0, 0x1234567890ABCDEF << 100, 5, 1, 2][:width]
    assert pa.permute(curve, st) == po.poseidon_permute(curve.fr, st, rf, rp)


@CURVES
def test_helper_at_width_3_is_the_width_3_helper(curve):
    st = pu.random_elems(curve, 3, 5)
    assert pa.permute(curve, st) == pu.permute(curve, st) and pa.hash(curve, st[:2]) == pu.hash2(curve, st[0], st[1])


# ---- zl_poseidon_spec -------------------------------------------------------------------------------------------------------------------------------
def test_spec_is_the_table():
    for arity, (width, rf, rp, tag) in pa.SPEC.items():
        assert poseidon_spec(arity) == {"arity": arity, "width": width, "full_rounds": rf, "partial_rounds": rp, "tag": tag}
    assert [poseidon_spec(a)["tag"] for a in pa.ARITIES] == [3, 7, 15, 31]
    for arity in (0, 1, 6):
        with pytest.raises(zb.BackendError) as e:
            poseidon_spec(arity)
        assert e.value.code == EINVAL
    L = zb.load_library()
    assert L.zl_poseidon_spec(3, None, None, None, None) == 0  # outputs are optional


# ---- zl_poseidon_constants --------------------------------------------------------------------------------------------------------------------------
@WIDTHS
def test_mds_equals_the_reference_matrices(width):
    _, mds = poseidon_constants(po.BLS12_381.cid, width)
    assert [[str(v) for v in pu.ints(row)] for row in mds] == FX["mds"][str(width)]


@CURVES
@WIDTHS
def test_constants_equal_the_oracle(curve, width):
    keys, mds = poseidon_constants(curve.cid, width)
    exp_keys, exp_mds = pa.constants(curve.name, width)
    rf, rp = pa.rounds(width)
    assert keys.shape == (width * (rf + rp), 4) and mds.shape == (width, width, 4)
    assert pu.ints(keys) == exp_keys
    assert [pu.ints(row) for row in mds] == exp_mds


def test_width_3_keys_are_the_reference_lfsr_values():
    keys, _ = poseidon_constants(po.BLS12_381.cid, 3)
    assert len(FX["lfsr_values"]) == 189 and [str(v) for v in pu.ints(keys)] == [str(v) for v in FX["lfsr_values"]]


def test_constants_refuse_unknown_widths_and_curves():
    L = zb.load_library()
    buf = np.zeros((6 * 64 + 36, 4), dtype=np.uint64)
    for width in (0, 2, 7):
        assert L.zl_poseidon_constants(po.BLS12_381.cid, width, zb._p64(buf), zb._p64(buf)) == EINVAL
    assert L.zl_poseidon_constants(99, 4, zb._p64(buf), zb._p64(buf)) == EINVAL


# ---- zl_poseidon_permute_w --------------------------------------------------------------------------------------------------------------------------
@CURVES
@WIDTHS
def test_permute_w_equals_the_model(curve, width):
    vals = pu.random_elems(curve, 4 * width, 31 + width)
    states = [vals[width * i:width * (i + 1)] for i in range(4)] + pa.edge_states(curve, width)
    for st in states:
        got = poseidon_permute(curve.cid, pu.limbs(st))
        assert got.shape == (width, 4) and pu.ints(got) == pa.permute(curve, st), st


@CURVES
def test_permute_w_at_width_3_is_zl_poseidon_permute(curve):
    L = zb.load_library()
    for st in [pu.random_elems(curve, 3, 41), [3, 1, 2], [curve.fr.p - 1] * 3]:
        a, b = pu.limbs(st), pu.limbs(st)
        assert L.zl_poseidon_permute_w(curve.cid, 3, zb._p64(a)) == 0 and L.zl_poseidon_permute(curve.cid, zb._p64(b)) == 0
        assert a.tobytes() == b.tobytes()


def test_permute_w_of_3_1_2_is_the_reference_vector():
    L = zb.load_library()
    st = pu.limbs([3, 1, 2])
    assert L.zl_poseidon_permute_w(po.BLS12_381.cid, 3, zb._p64(st)) == 0
    assert [str(v) for v in pu.ints(st)] == FX["permutation_width3"]["output"]


def test_permute_w_refuses_unknown_widths_and_curves():
    L = zb.load_library()
    st = np.zeros((8, 4), dtype=np.uint64)
    for width in (2, 7):
        assert L.zl_poseidon_permute_w(po.BLS12_381.cid, width, zb._p64(st)) == EINVAL
        with pytest.raises(zb.BackendError) as e:
            poseidon_permute(po.BN254.cid, np.zeros((width, 4), dtype=np.uint64))
        assert e.value.code == EINVAL
    assert L.zl_poseidon_permute_w(99, 4, zb._p64(st)) == EINVAL
    assert L.zl_poseidon_permute_w(po.BLS12_381.cid, 4, None) == EINVAL
    assert not st.any()


# ---- batched, ctx == NULL ---------------------------------------------------------------------------------------------------------------------------
@CURVES
@ARITIES
def test_hash_is_lane_0_of_the_tagged_permutation(curve, arity):
    width = arity + 1
    vals = pu.random_elems(curve, 5 * arity, 51 + arity)
    inputs = [vals[arity * i:arity * (i + 1)] for i in range(5)] + [[curve.fr.p - 1] * arity, [0] * arity]
    got = zb.poseidon_hash_host(curve.cid, states3d(inputs))
    assert got.shape == (len(inputs), 4)
    tagged = [[(1 << arity) - 1] + x for x in inputs]
    assert pu.ints(got) == [pa.hash(curve, x) for x in inputs] == [pa.permute(curve, s)[0] for s in tagged]
    perm = zb.poseidon_permute_batch_host(curve.cid, states3d(tagged))
    assert perm.shape == (len(inputs), width, 4)
    assert [pu.ints(p) for p in perm] == [pa.permute(curve, s) for s in tagged]
    assert np.array_equal(perm[:, 0, :], got)


@CURVES
def test_arity_2_through_the_new_entry_points_is_hash2(curve):
    vals = pu.random_elems(curve, 12, 61)
    xy = pu.limbs(vals).reshape(6, 2, 4)
    assert zb.poseidon_hash_host(curve.cid, xy).tobytes() == zb.poseidon_hash2_host(curve.cid, xy).tobytes()
    L = zb.load_library()
    a, b = pu.limbs(vals).reshape(4, 3, 4).copy(), pu.limbs(vals).reshape(4, 3, 4).copy()
    assert L.zl_poseidon_permute_batch_w(None, curve.cid, 3, zb._p64(a), 4) == 0 and L.zl_poseidon_permute_batch(None, curve.cid, zb._p64(b), 4) == 0
    assert a.tobytes() == b.tobytes()


@CURVES
@ARITIES
def test_count_0_is_ok_and_r_is_refused(curve, arity):
    width = arity + 1
    assert zb.poseidon_hash_host(curve.cid, np.zeros((0, arity, 4), dtype=np.uint64)).shape == (0, 4)
    assert zb.poseidon_permute_batch_host(curve.cid, np.zeros((0, width, 4), dtype=np.uint64)).shape[0] == 0
    L = zb.load_library()
    assert L.zl_poseidon_hash_batch(None, curve.cid, arity, None, 0, None) == 0
    assert L.zl_poseidon_permute_batch_w(None, curve.cid, width, None, 0) == 0
    r = curve.fr.p
    base = pu.random_elems(curve, 3 * width, 71)
    for at in (0, 3 * arity - 1):
        vals = list(base[:3 * arity])
        vals[at] = r
        with pytest.raises(zb.BackendError) as e:
            zb.poseidon_hash_host(curve.cid, pu.limbs(vals).reshape(3, arity, 4))
        assert e.value.code == EINVAL
    for at in (0, 3 * width - 1):
        vals = list(base)
        vals[at] = r
        with pytest.raises(zb.BackendError) as e:
            zb.poseidon_permute_batch_host(curve.cid, pu.limbs(vals).reshape(3, width, 4))
        assert e.value.code == EINVAL
    vals = list(base)
    vals[-1] = r - 1  # the largest canonical value passes
    assert zb.poseidon_permute_batch_host(curve.cid, pu.limbs(vals).reshape(3, width, 4)).shape == (3, width, 4)


def test_batch_calls_refuse_unknown_arities_widths_and_null_pointers():
    L = zb.load_library()
    buf = np.zeros((16, 4), dtype=np.uint64)
    cid = po.BLS12_381.cid
    for arity in (1, 6):
        assert L.zl_poseidon_hash_batch(None, cid, arity, zb._p64(buf), 1, zb._p64(buf)) == EINVAL
        assert L.zl_poseidon_hash_batch_dev(None, cid, arity, None, 0, None) == EINVAL
    for width in (2, 7):
        assert L.zl_poseidon_permute_batch_w(None, cid, width, zb._p64(buf), 1) == EINVAL
    assert L.zl_poseidon_hash_batch(None, 99, 3, zb._p64(buf), 1, zb._p64(buf)) == EINVAL
    assert L.zl_poseidon_hash_batch(None, cid, 3, None, 1, zb._p64(buf)) == EINVAL
    assert L.zl_poseidon_hash_batch(None, cid, 3, zb._p64(buf), 1, None) == EINVAL
    assert L.zl_poseidon_permute_batch_w(None, cid, 4, None, 1) == EINVAL
    assert L.zl_poseidon_hash_batch_dev(None, cid, 3, zb._p64(buf), 1, zb._p64(buf)) == EINVAL  # the device-pointer form has no host path

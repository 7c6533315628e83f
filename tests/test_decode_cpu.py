"""The lane-uniform point decoders of csrc/zl_decode.h (what the device kernels of zl_decode_dev.hip run), compiled for the host and driven through
zl_test_decode_points_host / zl_test_fq2_sqrt: every record of the shared set (decode_util.py) gives the words, the infinity byte and the status of the
existing host decoder zl_point_from_bytes, the finite valid ones the points of the Python restatement; the Fq2 square root agrees with the oracle's on
zero, real, purely imaginary, square and non-square inputs.  No GPU."""
import numpy as np
import pytest

import decode_util as du
import oracle_lib as ol
from oracle_lib import po
from openzl_amd.backend import hook_decode_points_host, hook_fq2_sqrt

CASES = [(c, g) for c in du.CURVES for g in (1, 2)]
IDS = [f"{c.name}-g{g}" for c, g in CASES]


@pytest.mark.parametrize("curve,group", CASES, ids=IDS)
def test_record_set_reaches_every_status(curve, group):
    """the set is what the issue of this decoder asks for, and the host decoder agrees with what each construction implies"""
    recs = du.records(curve, group)
    _, inf, st = du.expected(curve, group)
    labels = [lab for lab, _, _ in recs]
    assert 30 <= len(recs) <= 60
    for i, (lab, _, implied) in enumerate(recs):
        if implied is not None:
            assert st[i] == implied, (lab, st[i])
    assert {du.OK, du.EINVAL, du.ENOTCURVE} == set(int(s) for s in st)
    assert inf[labels.index("infinity")] == 1 and inf.sum() == 1
    assert ("outside_subgroup" in labels) == (not (curve.cid == 2 and group == 1))


@pytest.mark.parametrize("curve,group", CASES, ids=IDS)
def test_host_build_of_the_decoders_equals_the_host_codec(curve, group):
    recs = du.records(curve, group)
    exy, einf, est = du.expected(curve, group)
    xy, inf, st = hook_decode_points_host(curve.cid, group, b"".join(r for _, r, _ in recs), len(recs))
    for i, (lab, _, _) in enumerate(recs):
        assert st[i] == est[i] and inf[i] == einf[i] and (xy[i] == exy[i]).all(), (i, lab, st[i], est[i])
    nq = ol.nlq(curve)
    for i, (lab, rec, _) in enumerate(recs):
        if est[i] != du.OK:
            assert not xy[i].any() and inf[i] == 0, lab
        elif not einf[i]:
            v = ol.limbs_to_ints(xy[i].reshape(2 * group, nq))
            P = (v[0], v[1]) if group == 1 else ((v[0], v[1]), (v[2], v[3]))
            assert P == (po.g1_decompress(curve, rec) if group == 1 else po.g2_decompress(curve, rec)), lab
            assert du.in_subgroup(curve, group, P), lab
    # one record alone, and none
    xy1, inf1, st1 = hook_decode_points_host(curve.cid, group, recs[0][1], 1)
    assert st1[0] == est[0] and (xy1[0] == exy[0]).all() and inf1[0] == einf[0]
    assert hook_decode_points_host(curve.cid, group, b"", 0)[2].size == 0


@pytest.mark.parametrize("curve", du.CURVES, ids=lambda c: c.name)
def test_fq2_sqrt_host(curve):
    vals = du.sqrt_inputs(curve)
    roots, ok = hook_fq2_sqrt(None, curve.cid, du.fq2_words(curve, vals))
    du.check_sqrt(curve, vals, roots, ok)
    assert ok[:9].all() and ok[9:15].all() and not ok[15:].any()  # every value with a zero component is a square of Fq2 (u^2 = -1, -1 a non-residue)

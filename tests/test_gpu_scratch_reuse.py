"""The device scratch slots of one ctx (csrc/zl_ctx.h: the zl_slot map) across calls of different kinds and growing sizes: four-lane MSM batches on G1 and G2
(four buffer sets side by side, each with its own sort temporaries and endomorphism image), a device product of pairings and two-pass transforms (the
scratch vector is the first set's second sort temporary) on a fresh ctx: small, then large enough that the slots have to grow, then the small inputs again.
Every result of every round against the oracle; the third round byte-equal to the first."""
import ctypes as C

import numpy as np
import pytest

import groth16_util as gu
import oracle_lib as ol
from oracle_lib import po
from openzl_amd import ZL_G2, pairing

pytestmark = pytest.mark.gpu

CURVE = po.BLS12_381
JOBS = 4
SMALL = dict(log_msm=10, pairs=3, log_ntt=11)  # rounds 1 and 3
LARGE = dict(log_msm=12, pairs=5, log_ntt=13)  # round 2


def _oracle_msm_g2(bases, scalars):
    out = np.zeros(4 * ol.nlq(CURVE), dtype=np.uint64)
    inf = C.c_uint8(0)
    assert ol.lib().zlo_msm_g2(CURVE.cid, ol.p64(bases), 0, ol.p64(scalars), scalars.shape[0], 0, 8, ol.p64(out), C.byref(inf)) == 0
    return out, inf.value


def _product_of_singles(P, Q):
    ctx = po.Fq12Ctx(CURVE)
    acc = [1] + [0] * 11
    for i in range(P.shape[0]):
        acc = ctx.mul(acc, ol.limbs_to_ints(pairing(CURVE.cid, P[i], Q[i])))
    return acc


@pytest.fixture(scope="module")
def cases():
    """inputs and oracle results of the two sizes; the small case is a prefix of the large one's bases, so one handle per group serves all rounds (the
    endomorphism images kept with a handle belong to the first range used: the large round computes its own in the sets' slots)"""
    n_max = 1 << LARGE["log_msm"]
    B1 = ol.oracle_g1_mul_gen(CURVE, ol.random_scalars(CURVE, n_max, 7101))
    B2 = gu.g2_mul_gen(CURVE, ol.limbs_to_ints(ol.random_scalars(CURVE, n_max, 7102)))
    out = {"B1": B1, "B2": B2}
    for name, sz in (("small", SMALL), ("large", LARGE)):
        n = 1 << sz["log_msm"]
        S = [ol.random_scalars(CURVE, n, 7110 + 10 * sz["log_msm"] + j) for j in range(JOBS)]
        S[1][: n // 4] = ol.ints_to_limbs([1], 4)[0]  # the scalar-1 list differs per job
        S[2][n // 2:] = 0
        P = ol.oracle_g1_mul_gen(CURVE, ol.random_scalars(CURVE, sz["pairs"], 7200 + n))
        Q = gu.g2_mul_gen(CURVE, ol.limbs_to_ints(ol.random_scalars(CURVE, sz["pairs"], 7300 + n)))
        x = ol.random_scalars(CURVE, 1 << sz["log_ntt"], 7400 + n)
        out[name] = dict(
            n=n, S=S, P=P, Q=Q, x=x,
            g1=[ol.oracle_msm_g1(CURVE, B1[:n], s, algo=0, threads=8) for s in S],
            g2=[_oracle_msm_g2(B2[:n], s) for s in S],
            pp=_product_of_singles(P, Q),
            fwd=ol.oracle_ntt(CURVE, x),
            inv=ol.oracle_ntt(CURVE, x, inverse=True),
        )
    return out


def _round(backend, h1, h2, case):
    """one round on the backend; every result checked against the oracle and returned as bytes"""
    import torch

    n = case["n"]
    dev = [torch.from_numpy(s.view(np.int64)).cuda() for s in case["S"]]
    torch.cuda.synchronize()
    got = []
    for h, group, exp in ((h1, 1, case["g1"]), (h2, ZL_G2, case["g2"])):
        parts = backend.msm_batch_partial_dev(h, [t.data_ptr() for t in dev], n)
        for j in range(JOBS):
            xy, inf = backend.partials_sum(CURVE.cid, parts[j:j + 1], group=group)
            assert inf == exp[j][1] and (xy == exp[j][0]).all(), (group, j, n)
            got.append(xy.tobytes() + bytes([inf]))
    pp = backend.pairing_product(CURVE.cid, case["P"], case["Q"])
    assert ol.limbs_to_ints(pp) == case["pp"], n
    fwd = backend.ntt(CURVE.cid, case["x"])
    inv = backend.ntt(CURVE.cid, case["x"], inverse=True)
    assert (fwd == case["fwd"]).all() and (inv == case["inv"]).all(), n
    return got + [pp.tobytes(), fwd.tobytes(), inv.tobytes()]


def test_scratch_slots_grow_and_are_reused_across_call_kinds(backend, cases):
    from openzl_amd import Backend

    be = Backend(0)  # a fresh ctx beside the session's (which torch-initialises the device first): its slots start empty, so round 2 has to grow them
    try:
        h1 = be.bases_upload(CURVE.cid, cases["B1"])
        h2 = be.bases_upload(CURVE.cid, cases["B2"], group=ZL_G2)
        first = _round(be, h1, h2, cases["small"])
        _round(be, h1, h2, cases["large"])
        again = _round(be, h1, h2, cases["small"])
    finally:
        be.close()
    assert again == first

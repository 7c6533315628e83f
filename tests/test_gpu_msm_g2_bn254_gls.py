"""GPU: the endomorphism split of BN254 G2 plain MSMs (csrc/zl_msm_endo.h k_gls_split_lattice / k_gls_psi, constants from tools/gen_bn254_gls.py): four signed
64-bit quarter-scalars over P, psi(P), psi^2(P), psi^3(P).  The split kernel alone through zl_test_endo_split, MSMs over scalars on its decision boundaries
against the CPU oracle, and whole BN254 proofs."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import groth16_util as gu
import oracle_lib as ol
from oracle_lib import po
from openzl_amd import ZL_G2
from openzl_amd.backend import hook_endo_split

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gen():
    """tools/gen_bn254_gls.py as a module: lambda, the basis and its edge-scalar list"""
    spec = importlib.util.spec_from_file_location("gen_bn254_gls", os.path.join(ROOT, "tools", "gen_bn254_gls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _oracle_msm_g2(curve, bases, scalars, threads=8):
    out = np.zeros(4 * ol.nlq(curve), dtype=np.uint64)
    inf = C.c_uint8(0)
    assert ol.lib().zlo_msm_g2(curve.cid, ol.p64(bases), 0, ol.p64(scalars), scalars.shape[0], 0, threads, ol.p64(out), C.byref(inf)) == 0
    return out, inf.value


def _parts(rec):
    """(endo_k, n, 8) uint32 records -> signed Python integers [j][i]"""
    out = []
    for part in rec:
        row = []
        for w in part:
            assert not w[4:7].any() and (int(w[7]) & 0x7FFFFFFF) == 0
            mag = sum(int(w[a]) << (32 * a) for a in range(4))
            neg = int(w[7]) >> 31
            assert mag != 0 or not neg  # a zero magnitude carries no sign
            row.append(-mag if neg else mag)
        out.append(row)
    return out


def test_split_records_recombine(backend, gen):
    curve = po.BN254
    r, lam = curve.fr.p, gen.lam
    # (the tool's model runs 40 multiples of every lambda power and basis entry; 4 keep this test short -- every category is still there, as the next line checks)
    edge = gen.edge_scalars(4)
    assert {0, 1, r - 1, lam, lam**2 % r, lam**3 % r} <= set(edge) and any(e >= r for e in edge) and all(e < (1 << 254) for e in edge)
    ks = edge + ol.limbs_to_ints(ol.random_scalars(curve, 4096, 5501))
    n = len(ks)
    rec, bad, endo_k, bits = hook_endo_split(backend, curve.cid, ZL_G2, ol.ints_to_limbs(ks, 4))
    assert endo_k == 4 and bits == 64 and bad == 0 and rec.shape == (4, n, 8)
    parts = _parts(rec)
    for i, k in enumerate(ks):
        q = [parts[j][i] for j in range(4)]
        assert all(abs(v) < (1 << bits) for v in q), hex(k)
        assert (sum(v * lam**j for j, v in enumerate(q)) - k) % r == 0, hex(k)
    # every edge scalar alone (a grid of one lane), same records as inside the batch
    for i, k in enumerate(edge):
        rec1, bad1, k1, b1 = hook_endo_split(backend, curve.cid, ZL_G2, ol.ints_to_limbs([k], 4))
        assert (k1, b1, bad1) == (4, 64, 0) and (rec1[:, 0] == rec[:, i]).all(), hex(k)
    # scalars of bases at infinity are dropped; the others are unchanged by the flags
    inf = np.zeros(n, dtype=np.uint8)
    inf[[0, 3, len(edge) + 7, n - 1]] = 1
    rec_i, bad_i, _, _ = hook_endo_split(backend, curve.cid, ZL_G2, ol.ints_to_limbs(ks, 4), inf)
    assert bad_i == 0 and not rec_i[:, inf == 1].any() and (rec_i[:, inf == 0] == rec[:, inf == 0]).all()
    # a scalar with bit 254 or above cannot be canonical: bad bit 0
    for wide in ((1 << 254), (1 << 255) + 5, (1 << 256) - 1):
        _, badw, _, _ = hook_endo_split(backend, curve.cid, ZL_G2, ol.ints_to_limbs([3, wide, 7], 4))
        assert badw & 1, hex(wide)


def test_split_hook_reproduces_the_bls12_381_digits(backend):
    """the existing BLS12-381 G2 kernel through the same hook: base-|z| digits, odd digits negative"""
    curve = po.BLS12_381
    r, z = curve.fr.p, 0xD201000000010000
    edge = [0, 1, z - 1, z, z + 1, z * z - 1, z * z, z**3 - 1, z**3, (z - 1) * (1 + z + z * z + z**3) % r, r - 1, r - z, r, (1 << 255) - 1]
    ks = edge + ol.limbs_to_ints(ol.random_scalars(curve, 1000, 5502))
    rec, bad, endo_k, bits = hook_endo_split(backend, curve.cid, ZL_G2, ol.ints_to_limbs(ks, 4))
    assert (endo_k, bits, bad) == (4, 64, 0)
    parts = _parts(rec)
    for i, k in enumerate(ks):
        k %= r
        for j in range(4):
            d = (k // z**j) % z
            assert parts[j][i] == (-d if j & 1 else d), (hex(k), j)
    _, badw, _, _ = hook_endo_split(backend, curve.cid, ZL_G2, ol.ints_to_limbs([1 << 255], 4))
    assert badw & 1


def test_msm_bn254_g2_gls_edge_scalars(backend, gen):
    """The BN254 twin of test_msm_g2_gls_edge_scalars: scalars on the split's decision boundaries beside random ones, a base at infinity, P = +-Q inside a bucket,
    through the LDS sort, the wide sort at c = 16, narrow windows and the fall-back to plain windows (c <= 3), single call and pipelined batch, a range that takes
    the per-call image copy, and every edge scalar alone."""
    import torch

    curve = po.BN254
    r = curve.fr.p
    edge = sorted({e % r for e in gen.edge_scalars(4)})  # (4 multiples instead of the model's 40, as above)
    n = 600  # inside the size gate of MsmJob::plan (csrc/zl_msm_job.h: BN254 G2 splits below 2^ZL_GLS_HOLE_LO_LOG = 2^11 points), like the one-point MSMs at the end
    assert len(edge) < n - 100
    _, _, endo_k, _ = hook_endo_split(backend, curve.cid, ZL_G2, ol.ints_to_limbs([5], 4))
    assert endo_k == 4
    S = ol.random_scalars(curve, n, 883)
    S[: len(edge)] = ol.ints_to_limbs(edge, 4)
    ks = ol.limbs_to_ints(ol.random_scalars(curve, n, 884))
    a = len(edge) + 10
    ks[a + 1] = ks[a]            # P = Q inside a bucket
    ks[a + 3] = r - ks[a + 2]    # P = -Q inside a bucket
    S[a + 1] = S[a]
    S[a + 3] = S[a + 2]
    B = gu.g2_mul_gen(curve, ks)
    B[40] = 0  # a base at infinity (under an edge scalar)
    h = backend.bases_upload(curve.cid, B, group=ZL_G2)
    exp, einf = _oracle_msm_g2(curve, B, S)
    d_s = torch.from_numpy(S.view(np.int64)).cuda()
    torch.cuda.synchronize()
    try:
        for c in (0, 4, 9, 16, 3):
            backend.set_msm_window(c)
            got, inf = backend.msm_dev(h, d_s.data_ptr(), n)
            assert inf == einf and (got == exp).all(), c
            if c == 0:
                # the job really ran on quarter-scalars: zl_pick_window's cost model (n W 1.1 + per-bucket W 2^(c-1)) has its minimum at c = 7 for 4 * 600 records
                # of 64 bits and at c = 6 for 600 scalars of 254 bits, so a job that planned plain windows reports 6
                assert backend.last_timing().window_bits == 7
        backend.set_msm_window(0)
        parts = backend.msm_batch_partial_dev(h, [d_s.data_ptr()] * 5, n)
        for j in range(5):
            xy, pinf = backend.partials_sum(curve.cid, parts[j:j + 1], group=ZL_G2)
            assert pinf == einf and (xy == exp).all(), j
        # another range of the handle than the one whose images are kept with it: the per-call copy
        for first, cnt in ((1, n - 1), (0, n), (7, 300)):
            got, inf = backend.msm(h, S[first:first + cnt], first=first)
            e2, i2 = _oracle_msm_g2(curve, B[first:first + cnt], S[first:first + cnt])
            assert inf == i2 and (got == e2).all(), (first, cnt)
        backend.set_msm_window(7)
        for e in edge:
            s1 = ol.ints_to_limbs([e], 4)
            got, inf = backend.msm(h, s1)
            e1, i1 = _oracle_msm_g2(curve, B[:1], s1, threads=1)
            assert inf == i1 and (got == e1).all(), hex(e)
    finally:
        backend.set_msm_window(0)
        backend.bases_free(h)


TD = po.Groth16Trapdoor(alpha=0x1111_2222_3333, beta=0x4444_5555_6666, gamma=0x7777_8888, delta=0x9999_AAAA_BBBB, tau=0xCCCC_DDDD_EEEE_F001)
R_, S_ = 0x1234_5678_9ABC_DEF0_1111, 0x0FED_CBA9_8765_4321_2222


@pytest.mark.parametrize("k", [1, 8])
def test_groth16_bn254_proof_unchanged_by_the_split(backend, k):
    """a BN254 Poseidon-chain proof (its B comes from a G2 MSM over the split scalars) is byte-equal to the oracle's"""
    curve = po.BN254
    cs = po.poseidon_chain_circuit(curve.fr, k)
    pk = gu.setup_with_trapdoor(curve, cs, TD)
    arrays = gu.r1cs_arrays(cs)
    z = ol.ints_to_limbs(cs.assignment(), 4)
    r = ol.ints_to_limbs([R_], 4)[0]
    s = ol.ints_to_limbs([S_], 4)[0]
    dpk = gu.upload_pk(backend, curve, pk)
    try:
        got = backend.groth16_prove(curve.cid, dpk, arrays, z, r, s)
    finally:
        gu.free_pk(backend, dpk)
    exp, _ = gu.oracle_prove(curve, arrays, z, pk, r, s, threads=8)
    assert len(got) == len(exp) == 6
    for g, e in zip(got, exp):
        assert np.array_equal(np.asarray(g), np.asarray(e))
        if np.ndim(g):
            assert np.asarray(g, dtype=np.uint64).tobytes() == np.asarray(e, dtype=np.uint64).tobytes()

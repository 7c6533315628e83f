"""GPU parity: zl_msm_multi_dev (many scalar vectors over one base range in one device pass, csrc/zl_msm_multi.hip) against zl_msm_dev per vector, byte for
byte, and against the CPU oracle for one vector per case.  The shapes are the smallest at which the kernels can go wrong: n around the 64 lanes of a wave,
n that is no multiple of it, counts around the 64 lanes of the per-vector kernels, several chunks, and a slice cut (n > 2048)."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
from oracle_lib import po
from openzl_amd import ZL_G1, ZL_G2, BackendError

pytestmark = pytest.mark.gpu
EINVAL, EHANDLE = -1, -5
GROUPS = [(po.BLS12_381, ZL_G1), (po.BLS12_381, ZL_G2), (po.BN254, ZL_G1), (po.BN254, ZL_G2)]
GID = lambda cg: f"{cg[0].name}-G{cg[1]}"  # noqa: E731
NB = 1100       # points of the shared handle
MAXC = 130      # vectors of the shared scalar matrix
P_AT, NEG_AT, REP_AT, INF_AT = 6, 7, 5, (3, 20)  # B[7] = -B[6], B[5] = B[4], B[3] = B[20] = infinity


def _oracle(curve, group, B, S):
    if group == ZL_G1:
        return ol.oracle_msm_g1(curve, B, S, algo=0, threads=8)
    out = np.zeros(4 * ol.nlq(curve), dtype=np.uint64)
    inf = C.c_uint8(0)
    assert ol.lib().zlo_msm_g2(curve.cid, ol.p64(np.ascontiguousarray(B)), 0, ol.p64(np.ascontiguousarray(S)), S.shape[0], 0, 8, ol.p64(out), C.byref(inf)) == 0
    return out, inf.value


def _neg(curve, group, pt):
    """-P on canonical limbs: every Fq component of y becomes q - c"""
    nl, q = ol.nlq(curve), curve.fq.p
    out = pt.copy()
    for comp in range(group, 2 * group):  # the components of y follow those of x
        c = ol.limbs_to_ints(pt[comp * nl:(comp + 1) * nl].reshape(1, -1))[0]
        out[comp * nl:(comp + 1) * nl] = ol.ints_to_limbs([(q - c) % q], nl)[0]
    return out


_CACHE = {}


def _setup(backend, curve, group):
    """One handle per (curve, group) for the whole module: NB points with repeated points, P next to -P and two encodings of infinity inside every tested range."""
    key = (curve.cid, group)
    if key not in _CACHE:
        h0 = backend.bases_generate(curve.cid, ol.random_scalars(curve, NB, 7100 + 10 * curve.cid + group), group=group)
        B = backend.bases_download(h0)
        backend.bases_free(h0)
        B[REP_AT] = B[REP_AT - 1]
        B[NEG_AT] = _neg(curve, group, B[P_AT])
        for i in INF_AT:
            B[i] = 0
        _CACHE[key] = (backend.bases_upload(curve.cid, B, group=group), B)
    return _CACHE[key]


def _device(S):
    import torch

    d = torch.from_numpy(np.ascontiguousarray(S).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return d


def _matrix(curve, n, count, stride, seed):
    """(count, stride, 4) scalars: rows j < n of every vector are canonical, the padding behind them is all ones (not a scalar: reading it would be flagged)"""
    S = np.full((count, stride, 4), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    if n:
        S[:, :n] = ol.random_scalars(curve, count * n, seed).reshape(count, n, 4)
    return S


def _each_dev(backend, h, d, n, count, stride, first):
    outs = [backend.msm_dev(h, d.data_ptr() + j * stride * 32, n, first=first) for j in range(count)]
    return np.stack([o[0] for o in outs]), np.array([o[1] for o in outs], dtype=np.uint8)


@pytest.mark.parametrize("cg", GROUPS, ids=GID)
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257, 1000])
def test_parity_per_vector(backend, cg, n):
    """count in {1, 2, 3, 65, 130} over bases [1, 1 + n) with a stride above n: every vector equals zl_msm_dev, vector 0 equals the oracle."""
    curve, group = cg
    h, B = _setup(backend, curve, group)
    first, stride = 1, n + 3
    S = _matrix(curve, n, MAXC, stride, 9000 + n)
    d = _device(S)
    exp, einf = _each_dev(backend, h, d, n, MAXC, stride, first)  # once: the vectors of a smaller count are the first ones of this matrix
    o_xy, o_inf = _oracle(curve, group, B[first:first + n], S[0, :n]) if n else (np.zeros_like(exp[0]), 1)
    assert einf[0] == o_inf and (exp[0] == o_xy).all()
    for count in (1, 2, 3, 65, 130):
        got, inf = backend.msm_multi_dev(h, d.data_ptr(), n, count, stride=stride, first=first)
        assert got.shape == exp[:count].shape
        assert (inf == einf[:count]).all() and (got == exp[:count]).all(), count
        assert inf[0] == o_inf and (got[0] == o_xy).all(), count


@pytest.mark.parametrize("cg", GROUPS, ids=GID)
def test_slice_cut(backend, cg):
    """n = 1100 over the whole handle stays in one slice; the fold over slices needs n > 2048, reached here by a handle of 2100 generated points."""
    curve, group = cg
    n, count = 2100, 3
    h = backend.bases_generate(curve.cid, ol.random_scalars(curve, n, 7300 + group), group=group)
    try:
        B = backend.bases_download(h)
        S = _matrix(curve, n, count, n, 7400 + group)
        d = _device(S)
        exp, einf = _each_dev(backend, h, d, n, count, n, 0)
        got, inf = backend.msm_multi_dev(h, d.data_ptr(), n, count)
        o_xy, o_inf = _oracle(curve, group, B, S[1])
    finally:
        backend.bases_free(h)
    assert (inf == einf).all() and (got == exp).all()
    assert inf[1] == o_inf and (got[1] == o_xy).all()


@pytest.mark.parametrize("cg", GROUPS, ids=GID)
def test_every_branch_of_the_addition(backend, cg):
    """All-zero, all-one and all-(r - 1) vectors, a single scalar in the last slot, one digit in every window (one bucket takes every point), random scalars
    with equal scalars on the repeated point and on P / -P, and a vector whose sum is infinity; over a range with repeated points, P beside -P and infinity
    bases.  Each against zl_msm_dev and the oracle."""
    curve, group = cg
    h, B = _setup(backend, curve, group)
    n, r = 300, curve.fr.p
    lim = lambda v: ol.ints_to_limbs([v], 4)[0]  # noqa: E731
    same_digit = sum(21 << (6 * w) for w in range(42))  # digit 21 in the 42 full windows, < 2^252 < r
    assert same_digit < r
    rnd = ol.random_scalars(curve, n, 8100 + group)
    rnd[REP_AT] = rnd[REP_AT - 1]
    rnd[NEG_AT] = rnd[P_AT]
    cancel = np.zeros((n, 4), dtype=np.uint64)
    cancel[P_AT] = cancel[NEG_AT] = rnd[11]
    cancel[INF_AT[0]] = rnd[12]
    last = np.zeros((n, 4), dtype=np.uint64)
    last[n - 1] = rnd[13]
    vecs = [np.zeros((n, 4), dtype=np.uint64), np.tile(lim(1), (n, 1)), np.tile(lim(r - 1), (n, 1)), last, np.tile(lim(same_digit), (n, 1)), rnd, cancel]
    S = np.ascontiguousarray(np.stack(vecs))
    d = _device(S)
    exp, einf = _each_dev(backend, h, d, n, len(vecs), n, 0)
    got, inf = backend.msm_multi_dev(h, d.data_ptr(), n, len(vecs))
    assert (inf == einf).all() and (got == exp).all()
    for j, v in enumerate(vecs):
        o_xy, o_inf = _oracle(curve, group, B[:n], v)
        assert inf[j] == o_inf and (got[j] == o_xy).all(), j
    assert inf[0] == 1 and inf[6] == 1 and not got[0].any() and not got[6].any()  # the two sums that are infinity
    assert inf[1] == 0 and inf[5] == 0


@pytest.mark.parametrize("cg", GROUPS, ids=GID)
def test_chunks_and_window_table(backend, cg):
    """count = 130 in four chunks (ZL_TUNE_MSM_MULTI_CHUNK = 40) gives the bytes of the single chunk; a handle with a window table gives the bytes of the plain one."""
    curve, group = cg
    h, B = _setup(backend, curve, group)
    n, count = 257, 130
    S = _matrix(curve, n, count, n, 8300 + group)
    d = _device(S)
    one, one_inf = backend.msm_multi_dev(h, d.data_ptr(), n, count, first=2)
    assert backend.last_timing().launches == 1
    os.environ["ZL_TUNE_MSM_MULTI_CHUNK"] = "40"
    try:
        got, inf = backend.msm_multi_dev(h, d.data_ptr(), n, count, first=2)
        assert backend.last_timing().launches == 4
    finally:
        del os.environ["ZL_TUNE_MSM_MULTI_CHUNK"]
    assert (inf == one_inf).all() and (got == one).all()
    j = 77
    o_xy, o_inf = _oracle(curve, group, B[2:2 + n], S[j])
    assert one_inf[j] == o_inf and (one[j] == o_xy).all()
    ht = backend.bases_upload(curve.cid, B, group=group)
    try:
        backend.bases_precompute(ht, 16)
        tab, tab_inf = backend.msm_multi_dev(ht, d.data_ptr(), n, count, first=2)
    finally:
        backend.bases_free(ht)
    assert (tab_inf == one_inf).all() and (tab == one).all()


def test_wide_scalar_is_refused(backend):
    """A scalar with bits at or above the scalar field's width is no canonical scalar: ZL_EINVAL, as from zl_msm_dev."""
    curve, group = po.BLS12_381, ZL_G1
    h, _ = _setup(backend, curve, group)
    S = _matrix(curve, 70, 3, 70, 8500)
    S[2, 69, 3] |= np.uint64(1 << 63)
    d = _device(S)
    with pytest.raises(BackendError) as e:
        backend.msm_dev(h, d.data_ptr() + 2 * 70 * 32, 70)
    assert e.value.code == EINVAL
    with pytest.raises(BackendError) as e:
        backend.msm_multi_dev(h, d.data_ptr(), 70, 3)
    assert e.value.code == EINVAL
    got, inf = backend.msm_multi_dev(h, d.data_ptr(), 70, 2)  # the two clean vectors alone are fine
    exp, einf = _each_dev(backend, h, d, 70, 2, 70, 0)
    assert (inf == einf).all() and (got == exp).all()


def test_argument_errors_launch_nothing(backend):
    """NULL pointers, a stride below n, a range past the end, an unknown handle and a lane's handle on its parent: the ABI's codes, and no launch -- the timing
    record of the last successful call (its chunk count) is still in place afterwards."""
    curve, group = po.BN254, ZL_G1
    h, _ = _setup(backend, curve, group)
    L, ctx = backend.L, backend._ctx
    n, count = 65, 5
    d = _device(_matrix(curve, n, count, n, 8600))
    out = np.zeros((count, 8), dtype=np.uint64)
    inf = np.zeros(count, dtype=np.uint8)
    u8p = C.POINTER(C.c_uint8)
    call = lambda c, hh, first, ds, nn, st, cnt, o: L.zl_msm_multi_dev(c, hh, first, C.c_void_p(ds), nn, st, cnt, o, inf.ctypes.data_as(u8p))  # noqa: E731
    os.environ["ZL_TUNE_MSM_MULTI_CHUNK"] = "2"
    try:
        assert call(ctx, h, 0, d.data_ptr(), n, n, count, ol.p64(out)) == 0
    finally:
        del os.environ["ZL_TUNE_MSM_MULTI_CHUNK"]
    assert backend.last_timing().launches == 3
    good = out.copy()
    assert call(None, h, 0, d.data_ptr(), n, n, count, ol.p64(out)) == EINVAL
    assert call(ctx, h, 0, None, n, n, count, ol.p64(out)) == EINVAL
    assert call(ctx, h, 0, d.data_ptr(), n, n, count, None) == EINVAL
    assert call(ctx, h, 0, d.data_ptr(), n, n - 1, count, ol.p64(out)) == EINVAL
    assert call(ctx, h, NB - n + 1, d.data_ptr(), n, n, count, ol.p64(out)) == EINVAL
    assert call(ctx, h, NB + 1, d.data_ptr(), 0, 0, count, ol.p64(out)) == EINVAL
    assert call(ctx, 0x7FFF123456, 0, d.data_ptr(), n, n, count, ol.p64(out)) == EHANDLE
    lane = backend.fork()
    try:
        hl = lane.bases_generate(curve.cid, ol.random_scalars(curve, n, 8601))
        assert call(ctx, hl, 0, d.data_ptr(), n, n, count, ol.p64(out)) == EHANDLE      # the lane's handle is not the parent's
        assert call(lane._ctx, h, 0, d.data_ptr(), n, n, count, ol.p64(out)) == 0       # the parent's handle read from the lane
        assert (out == good).all()
        lane.bases_free(hl)
    finally:
        backend._forks.remove(lane)
        lane.close()
    assert backend.last_timing().launches == 3 and (out == good).all()
    # nothing to do is not an error
    assert call(ctx, h, 0, None, n, n, 0, None) == 0
    assert call(ctx, h, 0, None, 0, 0, count, ol.p64(out)) == 0
    assert not out.any() and (inf == 1).all()
    assert call(ctx, h, NB, None, 0, 0, 1, ol.p64(out)) == 0

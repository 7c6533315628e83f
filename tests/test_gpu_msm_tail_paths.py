"""GPU parity for the tail and sort paths that depend on the BUCKET count, not on n: the merge by chunk boundaries (k_msm_merge_cuts reading the chunk heads the
accumulation left), the one-lane tree levels (adding blocks + copy blocks) and the wide sort whose recoder counts the first partition histogram.  A forced window of
17 or 20 bits has 2^20 .. 6.8 M buckets at any n, so a few thousand points reach all of them; with 8-entry chunks a bucket of 9+ entries is cut, one of more than 64
goes to the big list and one of more than 32 768 to the giant list.  Every case is compared with ol.oracle_msm_g1, bit-exact on canonical affine coordinates."""
import numpy as np
import pytest

import oracle_lib as ol
from oracle_lib import po

pytestmark = pytest.mark.gpu
CURVES = [po.BLS12_381, po.BN254]
N_MAX = (1 << 15) + 3
SIZES = [4000, 3 * 4096 + 1, N_MAX]  # 3 * 4096 + 1: four slices of 3073 scalars, no multiple of the recoder's 256-scalar steps
_cache = {}


def _bases(backend, curve):
    """N_MAX points k_i G per curve, generated once on the device (the generator is not under test here) and shared; the cases take prefixes."""
    if curve.name not in _cache:
        h = backend.bases_generate(curve.cid, ol.random_scalars(curve, N_MAX, 7001))
        _cache[curve.name] = backend.bases_download(h)
        backend.bases_free(h)
    return _cache[curve.name]


def _one(curve, v):
    return ol.ints_to_limbs([v], 4)[0]


def _check(backend, curve, c, B, S):
    exp, einf = ol.oracle_msm_g1(curve, B, S, algo=0, threads=8)
    h = backend.bases_upload(curve.cid, B)
    backend.set_msm_window(c)
    try:
        got, inf = backend.msm(h, S)
        assert backend.last_timing().window_bits == c
    finally:
        backend.set_msm_window(0)
        backend.bases_free(h)
    assert inf == einf and (got == exp).all()


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("c", [17, 20])
@pytest.mark.parametrize("n", SIZES)
def test_tail_paths_small_n(backend, curve, c, n):
    """uniform scalars with the edge values, a run of 200 equal scalars (25 chunks: big list) and one base at infinity"""
    B = _bases(backend, curve)[:n].copy()
    S = ol.random_scalars(curve, n, 7100 + c)
    S[0] = 0
    S[1] = _one(curve, 1)
    S[2] = _one(curve, curve.fr.p - 1)
    S[3] = _one(curve, 1 << (c - 1))        # digit exactly at the sign boundary
    S[4] = _one(curve, (1 << (c - 1)) + 1)  # first negative digit with a carry
    S[100:300] = S[100]
    B[5] = 0
    _check(backend, curve, c, B, S)


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("c", [17, 20])
def test_tail_paths_every_merge_form_in_one_call(backend, curve, c):
    """n = 2^15 + 3: a run of 3000 equal scalars (375 chunks: big list), runs of 2 .. 60 equal scalars (buckets cut once: two loads and one addition; cut into 3 .. 8
    chunks: the loop), uniform scalars for the rest"""
    n = N_MAX
    B = _bases(backend, curve)[:n]
    S = ol.random_scalars(curve, n, 7200 + c)
    S[1000:4000] = S[1000]
    at = 5000
    for run in range(2, 61):
        S[at:at + run] = S[at]
        at += run
    _check(backend, curve, c, B, S)


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("prefix", [16, 5], ids=["on-boundary", "inside-chunk"])
def test_tail_paths_cut_placement_one_bucket(backend, curve, prefix):
    """Scalars below 2^(c-1) have one non-zero digit, in window 0, so the sorted entry list IS the scalars' order by value: `prefix` scalars of value 6, then
    n - prefix of value 7.  Bucket 7 starts at entry `prefix` -- on a chunk boundary (16) or inside a chunk (5) -- and runs to the end of the list, whose last chunk
    holds 3 entries: every boundary's lane reads its chunk head, the first one owns the bucket (4095 chunks: big list; 4097: giant list)."""
    c, n = 20, N_MAX
    B = _bases(backend, curve)[:n]
    S = np.zeros((n, 4), dtype=np.uint64)
    S[:prefix, 0] = 6
    S[prefix:, 0] = 7
    _check(backend, curve, c, B, S)


@pytest.mark.parametrize("prefix", [8, 3, 0])
def test_tail_paths_cut_placement_short_buckets(backend, prefix):
    """As above with `prefix` single-entry buckets, then buckets of 12 equal scalars: with prefix 8 they start on a chunk boundary (8 + 4: cut once, head partial first)
    or in the middle of a chunk (4 + 8: cut once, ends with its chunk) in turn; with 3 and 0 they are cut once or twice at every offset.  The last bucket is short and
    the last chunk partial.  BN254 at n >= 2^13 keeps its plain scalars (no endomorphism split), so the digits are the ones written here."""
    curve, c, n = po.BN254, 20, 8192 + 11
    B = _bases(backend, curve)[:n]
    S = np.zeros((n, 4), dtype=np.uint64)
    S[:prefix, 0] = np.arange(1, prefix + 1, dtype=np.uint64)
    S[prefix:, 0] = prefix + 2 + np.arange(n - prefix, dtype=np.uint64) // 12  # (from prefix + 2: no scalar is 1, which would leave the sort for the scalar-1 list)
    _check(backend, curve, c, B, S)


def test_tail_paths_pipelined_batch_keeps_chunk_heads_apart(backend):
    """three jobs in flight on the three buffer sets, alternating two scalar vectors: every partial equals the single call's, and the first the oracle's"""
    import torch

    curve, c, n = po.BLS12_381, 20, N_MAX
    B = _bases(backend, curve)[:n]
    vecs = [ol.random_scalars(curve, n, 7300), ol.random_scalars(curve, n, 7301)]
    vecs[1][2000:5000] = vecs[1][2000]  # the second vector's cuts sit elsewhere
    dev = [torch.from_numpy(S.view(np.int64)).cuda() for S in vecs]
    torch.cuda.synchronize()
    exp, einf = ol.oracle_msm_g1(curve, B, vecs[0], algo=0, threads=8)
    h = backend.bases_upload(curve.cid, B)
    backend.set_msm_window(c)
    try:
        batch = backend.msm_batch_partial_dev(h, [dev[j % 2].data_ptr() for j in range(3)], n)
        single = [backend.msm_partial_dev(h, dev[j].data_ptr(), n) for j in range(2)]
    finally:
        backend.set_msm_window(0)
        backend.bases_free(h)
    for j in range(3):
        a, ai = backend.partials_sum(curve.cid, batch[j:j + 1])
        b, bi = backend.partials_sum(curve.cid, single[j % 2].reshape(1, -1))
        assert ai == bi and (a == b).all(), j
    got, inf = backend.partials_sum(curve.cid, batch[0:1])
    assert inf == einf and (got == exp).all()

"""The exact-cover window plan of split BLS12-381 G1 MSMs (csrc/zl_msm_cover_plan.h: widths 22, 21, 21, 21, 21, 22 over 15 uniform sets of 2^19 buckets, the split
inside the recoder k_msm_recode_cover, the per-set weights in MsmJob::finish), which the planner takes by itself only from 2^24 points on.  The test hook
(hook_msm_exact_cover) forces the same plan -- the same kernels and set layout -- at small n; every case first asks the plan hook that the job really runs on it.
Expected values: the CPU oracle's MSM on the very bases used, bit-exact on canonical affine words; at 2^20 points (sum s_i k_i) G from one oracle scalar
multiplication.  The host walk of the plan header under sanitizers is tests/test_msm_cover_plan.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
from oracle_lib import po
from openzl_amd.backend import hook_msm_batch_form, hook_msm_exact_cover, hook_msm_plan

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVE = po.BLS12_381
R = CURVE.fr.p
Z = 0xD201000000010000
LAM = Z * Z - 1
HALF = LAM >> 1
WIDTHS = (22, 21, 21, 21, 21, 22)
POS = tuple(sum(WIDTHS[:w]) for w in range(6))
N_MAX = 1 << 16
SEED_K, SEED_S = 24001, 24002
_cache = {}


def _edge_scalars():
    """0, 1, 2, r - 1, r - 2; the decision boundaries of the split; halves at +- their maximum; every window below the top at the tie 2^(w - 1) and one either side of
    it, as a positive and as a negative first half and as a second half; carry chains through all six windows"""
    assert LAM * LAM + LAM + 1 == R and sum(WIDTHS) == 128
    e = [0, 1, 2, R - 1, R - 2, LAM - 1, LAM, LAM + 1, HALF, HALF + 1, HALF - 1, HALF * LAM, (HALF + 1) * LAM, (HALF + 1) * LAM + HALF + 1, (HALF + 1) * LAM + HALF,
         HALF * LAM + HALF, HALF * LAM + HALF + 1, R - LAM, R - LAM - 1, (LAM + 1) * LAM, (HALF + 2) * LAM - 1, 3 * LAM, LAM * LAM]
    for a in (HALF + 1, HALF, -HALF, -(HALF + 1)):
        for b in (HALF + 1, HALF, -HALF, -(HALF + 1)):
            e.append(a + b * LAM)
    for w in range(5):
        for delta in (-1, 0, 1):
            m = ((1 << (WIDTHS[w] - 1)) + delta) << POS[w]
            e += [m, -m, m * LAM, -m * LAM, m + ((1 << POS[w]) - 1), -(m + ((1 << POS[w]) - 1))]
    chain = (1 << POS[5]) - 1
    e += [chain, -chain, chain * LAM, 3 * (1 << POS[5]) + chain, sum(((1 << (WIDTHS[w] - 1)) + 1) << POS[w] for w in range(5)),
          -sum(((1 << (WIDTHS[w] - 1)) + 1) << POS[w] for w in range(5))]
    return [x % R for x in e]


EDGE = _edge_scalars()
# the ones that also run alone (a one-point job on 7.9 M buckets costs a third of a second: its twelve entries are a long walk apart): one of each kind
_TIE = [((1 << (WIDTHS[w] - 1)) << POS[w]) for w in range(5)]
ALONE = [x % R for x in (1, 2, R - 1, (HALF + 1) * (1 + LAM), -(HALF + 1) * (1 + LAM), _TIE[0], -_TIE[4], _TIE[2] * LAM, ((1 << POS[5]) - 1) * LAM, -((1 << POS[5]) - 1))]
assert all(x in EDGE for x in ALONE)


def _neg(xy):
    """-P of a canonical affine G1 point"""
    nl = ol.nlq(CURVE)
    w = xy.reshape(-1, nl).copy()
    half = w.shape[0] // 2
    w[half:] = ol.ints_to_limbs([(CURVE.fq.p - v) % CURVE.fq.p for v in ol.limbs_to_ints(w[half:])], nl)
    return w.reshape(-1)


def _bases(backend):
    """N_MAX bases k_i G from the device generator (checked against the oracle in test_gpu_msm.py), with a point at infinity, a repeated and a negated point; the
    cases take prefixes.  Computed once."""
    if "B" not in _cache:
        h = backend.bases_generate(CURVE.cid, ol.random_scalars(CURVE, N_MAX, SEED_K))
        B = backend.bases_download(h)
        backend.bases_free(h)
        B[1] = 0                      # infinity (n = 2 has it too)
        B[7] = B[6]                   # a repeated point ...
        B[9] = _neg(B[8])             # ... and P beside -P
        B[40] = 0
        _cache["B"] = B
    return _cache["B"]


def _scalars(n, seed):
    """uniform scalars with the edge set in front (as much of it as fits), equal scalars on the repeated and on the negated point"""
    S = ol.random_scalars(CURVE, n, seed)
    m = min(n, len(EDGE))
    S[:m] = ol.ints_to_limbs(EDGE[:m], 4)
    if n > 9:
        S[7] = S[6]   # 2 s P: the bucket doubles
        S[9] = S[8]   # s P - s P: the bucket cancels
    return S


def _forced(backend):
    class _Ctx:
        def __enter__(self):
            self.old = hook_msm_exact_cover(backend, 1)

        def __exit__(self, *a):
            hook_msm_exact_cover(backend, self.old)
    return _Ctx()


def _assert_cover_plan(backend, h, n):
    p = hook_msm_plan(backend, h, n)
    assert p.glv == 1 and p.endo_k == 2 and p.c == 20 and p.W == 6 and p.SETS == 15 and p.NB == 15 << 19 and p.Gn == 240 and p.wide and not p.pre and p.spread_t == -1, p
    return p


def _run(backend, B, S):
    import torch

    n = S.shape[0]
    h = backend.bases_upload(CURVE.cid, np.ascontiguousarray(B[:n]))
    d = torch.from_numpy(np.ascontiguousarray(S).view(np.int64)).cuda()
    torch.cuda.synchronize()
    try:
        with _forced(backend):
            p = _assert_cover_plan(backend, h, n)
            got, inf = backend.msm_dev(h, d.data_ptr(), n)
    finally:
        backend.bases_free(h)
    return got, inf, p


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4097, N_MAX])
def test_exact_cover_matches_oracle(backend, n):
    """random and edge scalars over bases with infinity, a repeated and a negated point, at sizes around the wave, over one slice of the sort and at 2^16"""
    B = _bases(backend)
    S = _scalars(n, SEED_S + n)
    exp, einf = ol.oracle_msm_g1(CURVE, np.ascontiguousarray(B[:n]), S, algo=0, threads=8)
    got, inf, p = _run(backend, B, S)
    assert inf == einf and (got == exp).all(), p
    if n > 4096:
        assert p.nslices > 1 and p.by_cuts


def test_exact_cover_edge_scalars_alone(backend):
    """n = 1: one scalar of every kind of the edge set alone -- halves at +- their maximum, ties, carry chains, either sign, either half -- on a base that is not at
    infinity (the whole set runs inside the 4097- and 2^16-point cases above)"""
    import torch

    B = _bases(backend)
    b0 = np.ascontiguousarray(B[:1])
    S = ol.ints_to_limbs(ALONE, 4)
    d = torch.from_numpy(S.view(np.int64)).cuda()
    torch.cuda.synchronize()
    h = backend.bases_upload(CURVE.cid, b0)
    try:
        with _forced(backend):
            _assert_cover_plan(backend, h, 1)
            got = [backend.msm_dev(h, d.data_ptr() + 32 * i, 1) for i in range(len(ALONE))]
    finally:
        backend.bases_free(h)
    for i, e in enumerate(ALONE):
        e1, i1 = ol.oracle_msm_g1(CURVE, b0, S[i:i + 1])
        assert got[i][1] == i1 and (got[i][0] == e1).all(), hex(e)


@pytest.mark.parametrize("value", [R - 2, (HALF + 1) * LAM + HALF], ids=["r-2", "half-max"])
def test_exact_cover_all_equal_scalars(backend, value):
    """2^16 equal scalars: every window's entries of either half sit in ONE bucket of 65 536 entries -- 8192 chunks of 8, the giant-bucket path of the merge"""
    B = _bases(backend)
    S = np.ascontiguousarray(np.repeat(ol.ints_to_limbs([value], 4), N_MAX, axis=0))
    exp, einf = ol.oracle_msm_g1(CURVE, B, S, algo=0, threads=8)
    got, inf, p = _run(backend, B, S)
    assert p.may_giant and p.chunk * 4096 < N_MAX, p
    assert inf == einf and (got == exp).all()


def test_exact_cover_bad_scalar_is_refused(backend):
    """a scalar with bit 255 set is not canonical: the plan's recoder flags it like every other recoder, and the call fails instead of returning a sum"""
    from openzl_amd import BackendError

    B = _bases(backend)
    S = _scalars(64, 5)
    S[17, 3] |= np.uint64(1 << 63)
    with pytest.raises(BackendError):
        _run(backend, B, S)


_CHILD = r"""
import sys
import numpy as np
import torch
torch.cuda.init()
import oracle_lib as ol
from oracle_lib import po
from openzl_amd import Backend
from openzl_amd.backend import hook_msm_exact_cover, hook_msm_plan
curve = po.BLS12_381
n, seed_k, seed_a, seed_b = (int(x) for x in sys.argv[1:5])
be = Backend(0)
h = be.bases_generate(curve.cid, ol.random_scalars(curve, n, seed_k))
hook_msm_exact_cover(be, 1)
p = hook_msm_plan(be, h, n)
assert p.glv == 0 and p.endo_k == 1, p  # ZL_NO_GLV: never split, whatever the hook says
vecs = [ol.random_scalars(curve, n, s) for s in (seed_a, seed_b)]
dev = [torch.from_numpy(v.view(np.int64)).cuda() for v in vecs]
torch.cuda.synchronize()
parts = be.msm_batch_partial_dev(h, [dev[j % 2].data_ptr() for j in range(5)], n)
for j in range(5):
    xy, inf = be.partials_sum(curve.cid, parts[j:j + 1])
    print("RESULT", j, int(inf), xy.tobytes().hex())
be.bases_free(h)
be.close()
"""


def test_exact_cover_batch_of_five(backend, monkeypatch):
    """five MSMs alternating two scalar vectors at 2^16 points in one batch, on the three-stream pipeline (three rotating buffer sets: job 3 reuses job 0's) and on
    the side-by-side lanes: every partial equals the single call's, the oracle's, and the same batch of a process with ZL_NO_GLV set (plain windows)"""
    import torch

    n = N_MAX
    k = ol.random_scalars(CURVE, n, SEED_K)
    h = backend.bases_generate(CURVE.cid, k)
    vecs = [ol.random_scalars(CURVE, n, s) for s in (SEED_S + 1, SEED_S + 2)]
    dev = [torch.from_numpy(v.view(np.int64)).cuda() for v in vecs]
    torch.cuda.synchronize()
    try:
        B = backend.bases_download(h)
        exp = [ol.oracle_msm_g1(CURVE, B, v, algo=0, threads=8) for v in vecs]
        with _forced(backend):
            _assert_cover_plan(backend, h, n)
            single = [backend.partials_sum(CURVE.cid, backend.msm_partial_dev(h, d.data_ptr(), n).reshape(1, -1)) for d in dev]
            for j in range(2):
                assert single[j][1] == exp[j][1] and (single[j][0] == exp[j][0]).all(), j
            for knobs, side in (({"ZL_TUNE_SIDE_BY_SIDE_LOG": "0"}, False), ({}, True)):
                with monkeypatch.context() as m:
                    m.delenv("ZL_TUNE_SIDE_BY_SIDE_LOG", raising=False)
                    for name, v in knobs.items():
                        m.setenv(name, v)
                    assert hook_msm_batch_form(5, n)["side"] == side
                    for rep in range(2):
                        parts = backend.msm_batch_partial_dev(h, [dev[j % 2].data_ptr() for j in range(5)], n)
                        for j in range(5):
                            xy, inf = backend.partials_sum(CURVE.cid, parts[j:j + 1])
                            assert inf == single[j % 2][1] and xy.tobytes() == single[j % 2][0].tobytes(), (side, rep, j)
    finally:
        backend.bases_free(h)
    env = dict(os.environ, ZL_NO_GLV="1", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    env.pop("ZL_TUNE_SIDE_BY_SIDE_LOG", None)
    out = subprocess.run([sys.executable, "-c", _CHILD, str(n), str(SEED_K), str(SEED_S + 1), str(SEED_S + 2)], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    rows = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    assert [int(r[1]) for r in rows] == list(range(5)), out.stdout[-2000:]
    for r in rows:
        j = int(r[1])
        assert int(r[2]) == single[j % 2][1] and bytes.fromhex(r[3]) == single[j % 2][0].tobytes(), j


def test_exact_cover_known_discrete_log_2_20(backend):
    """2^20 points k_i G on the forced plan: the result is (sum s_i k_i mod r) G, one scalar multiplication of the CPU oracle"""
    import torch

    from openzl_amd.selfcheck import dot_mod_r

    n = 1 << 20
    k = ol.random_scalars(CURVE, n, 24020)
    S = ol.random_scalars(CURVE, n, 24021)
    S[5] = 0
    S[6] = ol.ints_to_limbs([1], 4)[0]
    S[7] = ol.ints_to_limbs([R - 1], 4)[0]
    h = backend.bases_generate(CURVE.cid, k)
    d = torch.from_numpy(S.view(np.int64)).cuda()
    torch.cuda.synchronize()
    try:
        with _forced(backend):
            p = _assert_cover_plan(backend, h, n)
            assert p.chunk * p.nchunks >= 12 * n > p.chunk * (p.nchunks - 1)  # twelve entries per point
            got, inf = backend.msm_dev(h, d.data_ptr(), n)
    finally:
        backend.bases_free(h)
    exp = ol.oracle_g1_mul_gen(CURVE, ol.ints_to_limbs([dot_mod_r(S, k, R)], 4))[0]
    assert not inf and (got == exp).all()


def test_planner_keeps_small_jobs_off_the_plan(backend):
    """without the hook a 2^16-point job is not planned on the exact cover (the picker's threshold is 2^24 points), and hook mode -1 forbids it"""
    B = _bases(backend)
    h = backend.bases_upload(CURVE.cid, np.ascontiguousarray(B))
    try:
        assert hook_msm_exact_cover(backend, 0) == 0
        p = hook_msm_plan(backend, h, N_MAX)
        assert p.glv == 1 and (p.W, p.SETS) != (6, 15) and p.W == p.SETS, p
        assert hook_msm_exact_cover(backend, -1) == 0
        q = hook_msm_plan(backend, h, N_MAX)
        assert hook_msm_exact_cover(backend, 0) == -1
        assert (q.c, q.W, q.SETS, q.glv) == (p.c, p.W, p.SETS, p.glv)
        with _forced(backend):
            backend.set_msm_window(18)  # a forced window keeps its uniform windows
            try:
                f = hook_msm_plan(backend, h, N_MAX)
            finally:
                backend.set_msm_window(0)
            assert f.c == 18 and f.W == f.SETS, f
    finally:
        backend.bases_free(h)

"""Every launch form of an MSM (MsmJob::plan_as, csrc/zl_msm_job.h) and of the batch driver (msm_run_jobs_t, csrc/zl_msm.hip) at a few thousand points, on all four
groups.  Almost every choice of the planner follows the SIZE of the job, so the workload reaches most forms only at millions of points; here a forced window
(set_msm_window) and the planner's own ZL_TUNE_* knobs select them at small n.  Every case first asks the plan hook (hook_msm_plan: MsmJob::plan alone, under the
same window and environment) and asserts the fields it exists for, so a change of the planner fails the case instead of emptying it.  Expected values: the CPU
oracle on the very bases used (ol.oracle_msm_g1, zlo_msm_g2), bit-exact on canonical affine words; the runs of one case under different knobs must be byte-equal too.

decision -> test
  (a) G2 merge by chunk boundaries (k_msm_merge_cuts_pair): buckets cut once / into 3..8 chunks, big list, giant list, cut on / inside a chunk, partial last chunk;
      one-lane-pair level 0 and tree                       -> test_g2_cut_buckets_every_merge_form, test_g2_cut_placement_one_bucket (big, giant),
                                                              test_g2_cut_placement_short_buckets
  (b) chunk length 8 / 16 / 32 / 64 / 128                  -> test_chunk_lengths
  (c) big_span 64 against 8 (nchunks > 2^17), G1           -> test_g1_big_span_64
  (d) accumulation: four / eight lanes against one lane / a lane pair per chunk              -> test_accumulation_forms
  (e) tail: by_cuts and one-lane levels on a small bucket count; per-bucket merge and four- / eight-lane levels on a large one; the single-chunk merge
                                                           -> test_tail_one_lane_on_few_buckets, test_tail_quad_on_many_buckets, test_tail_single_chunk_merge
  (f) red_g0 2 / 4 / 8: shortened by a narrow spread top window, spread_t == 0, no spread, clamped to H                       -> test_reduction_block_lengths
  (g) LDS sort: one-block prefix against the three-kernel scan, 1 / 4 / 64 scatter ranges, ragged n                          -> test_lds_sort_prefix_and_ranges
  (h) wide sort: one slice / several, 256 / 512 / 1024 threads, oversized sub-groups (k_msm_fine_sort_big), window and table -> test_wide_sort_forms
  (i) batch: three-stream pipeline against side-by-side lanes (1 / 2 / 3 / 4 lanes), phase-major issue  -> test_pipeline_small_batches, test_side_by_side_lanes_and_phases
  (j) heterogeneous jobs on the pipeline (one Groth16 proof)                                 -> test_groth16_proof_on_the_pipeline
  (k) ZL_TUNE_BATCH_INV 1 / 7 / 64 (batched inversion of bases_generate / download)          -> test_batch_inversion_lengths

Scalars below 2^(c-1) have one non-zero digit, in window 0, so the sorted entry list is the scalars' order by value; where the job runs on split scalars (`glv` of the
plan) the case asserts with hook_endo_split that those scalars split to (k, 0, ..), which leaves the list as it is.  Equal scalars split to equal parts, so a run of
equal scalars is a run of equal digits in every window of a split job as well."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import groth16_util as gu
import oracle_lib as ol
from oracle_lib import po
from openzl_amd import ZL_G1, ZL_G2, Circuit, Groth16Keys
from openzl_amd.backend import hook_endo_split, hook_msm_batch_form, hook_msm_plan

pytestmark = pytest.mark.gpu

CURVES = [po.BLS12_381, po.BN254]
GROUPS = [(po.BLS12_381, ZL_G1), (po.BN254, ZL_G1), (po.BLS12_381, ZL_G2), (po.BN254, ZL_G2)]
N_MAX = (1 << 15) + 3                 # G1, and the one giant-list case on G2
N_OF = {ZL_G1: N_MAX, ZL_G2: (1 << 13) + 11}
GIANT_SPAN = 4096                     # ZL_GIANT_SPAN (csrc/zl_msm_common.h): a bucket cut into more chunks goes to the giant list
KNOBS = ["ZL_TUNE_" + k for k in ("CHUNK", "SEG", "RANGES", "FS", "FS_CAP", "QUAD_ACC_CHUNKS", "QUAD_LANES", "SIDE_BY_SIDE_LOG", "SIDE_LANES", "PHASED_MIN_LOG",
                                  "BATCH_INV", "ENDO_CACHE_MB", "G16_FOLD_LOG_N")]
ABOVE_ALL = 1 << 30                   # a lane / chunk threshold above any count of this file
_points = {}


def _gid(g):
    return f"{g[0].name}-g{g[1]}"


def _pts(backend, g):
    """N_MAX points k_i G of the group, generated once on the device (the generator has its own test, (k)) and shared; the cases take prefixes."""
    if _gid(g) not in _points:
        h = backend.bases_generate(g[0].cid, ol.random_scalars(g[0], N_MAX, 8101 + g[1]), group=g[1])
        _points[_gid(g)] = backend.bases_download(h)
        backend.bases_free(h)
    return _points[_gid(g)]


def _neg(curve, xy):
    """-P of a canonical affine point: every Fq component of y negated"""
    nl = ol.nlq(curve)
    w = xy.reshape(-1, nl).copy()
    half = w.shape[0] // 2
    w[half:] = ol.ints_to_limbs([(curve.fq.p - v) % curve.fq.p for v in ol.limbs_to_ints(w[half:])], nl)
    return w.reshape(-1)


def _inputs(backend, g, n, seed, c):
    """n bases and uniform scalars with the edge set: 0, 1, r - 1, the digit at the sign boundary and the first negative digit with a carry, one base at infinity, a
    repeated point in one bucket (a doubling) and P next to -P in one bucket (a cancellation)"""
    curve = g[0]
    B = _pts(backend, g)[:n].copy()
    S = ol.random_scalars(curve, n, seed)
    S[0] = 0
    S[1:5] = ol.ints_to_limbs([1, curve.fr.p - 1, 1 << (c - 1), (1 << (c - 1)) + 1], 4)
    B[5] = 0
    B[7], S[7] = B[6], S[6]
    B[9], S[9] = _neg(curve, B[8]), S[8]
    return B, S


def _runs(S, at, lengths):
    """runs of equal scalars of the given lengths from index `at` on; returns the index behind them"""
    for run in lengths:
        S[at:at + run] = S[at]
        at += run
    assert at <= S.shape[0]
    return at


def _oracle(g, B, S):
    if g[1] == ZL_G1:
        return ol.oracle_msm_g1(g[0], B, S, algo=0, threads=8)
    out = np.zeros(4 * ol.nlq(g[0]), dtype=np.uint64)
    inf = C.c_uint8(0)
    assert ol.lib().zlo_msm_g2(g[0].cid, ol.p64(np.ascontiguousarray(B)), 0, ol.p64(np.ascontiguousarray(S)), S.shape[0], 0, 8, ol.p64(out), C.byref(inf)) == 0
    return out, inf.value


@contextlib.contextmanager
def _env(monkeypatch, knobs):
    """exactly the given knobs (names without ZL_TUNE_) set, every other planner knob unset"""
    with monkeypatch.context() as m:
        for k in KNOBS:
            m.delenv(k, raising=False)
        for k, v in knobs.items():
            assert "ZL_TUNE_" + k in KNOBS
            m.setenv("ZL_TUNE_" + k, str(v))
        yield


class _Case:
    """one (bases, scalars, window) input: uploaded once, its oracle value computed once, run under any number of knob settings"""

    def __init__(self, backend, monkeypatch, g, B, S, c=0, table=0, expect=True):
        self.be, self.mp, self.g, self.c, self.S, self.n = backend, monkeypatch, g, c, np.ascontiguousarray(S), S.shape[0]
        self.exp = _oracle(g, B, S) if expect else None
        self.h = backend.bases_upload(g[0].cid, np.ascontiguousarray(B), group=g[1])
        if table:
            backend.bases_precompute(self.h, table)
        self.results = []

    def plan(self, knobs):
        with _env(self.mp, knobs):
            self.be.set_msm_window(self.c)
            try:
                return hook_msm_plan(self.be, self.h, self.n)
            finally:
                self.be.set_msm_window(0)

    def run(self, knobs, want):
        """plan under `knobs`, assert want(plan), run the MSM under the same knobs, compare with the oracle and with every earlier run of the case"""
        with _env(self.mp, knobs):
            self.be.set_msm_window(self.c)
            try:
                p = hook_msm_plan(self.be, self.h, self.n)
                assert want(p), (knobs, p)
                got, inf = self.be.msm(self.h, self.S)
                if self.c:
                    assert self.be.last_timing().window_bits == self.c == p.c
            finally:
                self.be.set_msm_window(0)
        assert inf == self.exp[1] and (got == self.exp[0]).all(), (knobs, p)
        for other, oinf in self.results:
            assert inf == oinf and got.tobytes() == other.tobytes(), knobs
        self.results.append((got, inf))
        return p

    def close(self):
        self.be.bases_free(self.h)


@contextlib.contextmanager
def _case(*a, **kw):
    case = _Case(*a, **kw)
    try:
        yield case
    finally:
        case.close()


def _assert_first_part_only(backend, g, values):
    """the split in front of the group's plain MSM leaves these small scalars as (k, 0, ..): one entry per scalar, the digits written by the test"""
    S = ol.ints_to_limbs(list(values), 4)
    rec, bad, k, _ = hook_endo_split(backend, g[0].cid, g[1], S)
    assert bad == 0 and k in (2, 4)
    assert (rec[0, :, :2].copy().view(np.uint64)[:, 0] == S[:, 0]).all() and not rec[0, :, 2:].any()
    assert not (rec[1:] & np.uint32(0x7FFFFFFF)).any() and not (rec[1:, :, :7]).any()


# ------------------------------------------------------------------------------------------------ (a) G2 twin of test_gpu_msm_tail_paths.py
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("c", [16, 17, 20])
def test_g2_cut_buckets_every_merge_form(backend, monkeypatch, curve, c):
    """uniform scalars with the edge set, a run of 200 equal scalars (25 chunks of 8: big list) and runs of 2 .. 60 equal scalars (buckets cut once: two loads and one
    addition; cut into 3 .. 8 chunks: the loop), through k_msm_merge_cuts_pair, k_msm_merge_big_pair and the lane-pair level 0 and tree"""
    g = (curve, ZL_G2)
    B, S = _inputs(backend, g, N_OF[ZL_G2], 8200 + c, c)
    _runs(S, _runs(S, 100, [200]), range(2, 61))
    with _case(backend, monkeypatch, g, B, S, c=c) as case:
        p = case.run({}, lambda p: p.by_cuts and p.chunk == 8 and p.big_span == 8 and p.may_big and p.NB > p.tail_quad_max and not p.pre)
        assert 200 > p.big_span * p.chunk + p.chunk and 60 <= p.big_span * p.chunk


def _one_bucket(n, prefix):
    S = np.zeros((n, 4), dtype=np.uint64)
    S[:prefix, 0] = 6
    S[prefix:, 0] = 7
    return S


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("prefix", [16, 5], ids=["on-boundary", "inside-chunk"])
def test_g2_cut_placement_one_bucket(backend, monkeypatch, curve, prefix):
    """`prefix` scalars of value 6, then n - prefix of value 7: bucket 7 starts at entry `prefix` -- on a chunk boundary or inside a chunk -- and runs to the end of the
    list, whose last chunk is partial: every boundary's lane pair searches its bucket, the first one owns it (about 1025 chunks: big list)"""
    g, c, n = (curve, ZL_G2), 20, N_OF[ZL_G2]
    with _case(backend, monkeypatch, g, _pts(backend, g)[:n], _one_bucket(n, prefix), c=c) as case:
        p = case.run({}, lambda p: p.by_cuts and p.chunk == 8 and p.may_big and n % p.chunk != 0 and (prefix % p.chunk == 0) == (prefix == 16))
        chunks = (n - 1) // p.chunk - prefix // p.chunk + 1
        assert p.big_span < chunks <= GIANT_SPAN
        if p.glv:
            _assert_first_part_only(backend, g, [6, 7])


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_g2_cut_placement_one_bucket_giant(backend, monkeypatch, curve):
    """as above at n = 2^15 + 3: the bucket is cut into 4097 chunks and goes to the giant list (k_msm_merge_giant_pair / _giant2_pair)"""
    g, c, n, prefix = (curve, ZL_G2), 20, N_MAX, 5
    with _case(backend, monkeypatch, g, _pts(backend, g)[:n], _one_bucket(n, prefix), c=c) as case:
        p = case.run({}, lambda p: p.by_cuts and p.chunk == 8 and p.may_giant and n % p.chunk != 0)
        assert (n - 1) // p.chunk - prefix // p.chunk + 1 > GIANT_SPAN
        if p.glv:
            _assert_first_part_only(backend, g, [6, 7])


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("prefix", [8, 3, 0])
def test_g2_cut_placement_short_buckets(backend, monkeypatch, curve, prefix):
    """`prefix` single-entry buckets, then buckets of 12 equal scalars: with prefix 8 they start on a chunk boundary (8 + 4: cut once, head partial first) or in the
    middle of a chunk (4 + 8: cut once, ends with its chunk) in turn; with 3 and 0 they are cut once or twice at every offset.  The last chunk is partial."""
    g, c, n = (curve, ZL_G2), 20, N_OF[ZL_G2]
    S = np.zeros((n, 4), dtype=np.uint64)
    S[:prefix, 0] = np.arange(1, prefix + 1, dtype=np.uint64) + 1  # (from 2: no scalar is 1, which would leave the sort for the scalar-1 list)
    S[prefix:, 0] = prefix + 2 + np.arange(n - prefix, dtype=np.uint64) // 12
    with _case(backend, monkeypatch, g, _pts(backend, g)[:n], S, c=c) as case:
        p = case.run({}, lambda p: p.by_cuts and p.chunk == 8 and n % p.chunk != 0 and int(S[:, 0].max()) < (1 << (p.c - 1)))
        if p.glv:
            _assert_first_part_only(backend, g, np.unique(S[:, 0]).tolist())


# ------------------------------------------------------------------------------------------------ (b) chunk length
@pytest.mark.parametrize("g", GROUPS, ids=_gid)
def test_chunk_lengths(backend, monkeypatch, g):
    """the mixed input of (a) at c = 17 with 8-, 16-, 32-, 64- and 128-entry chunks.  A run of 8 * 128 + 128 + 5 equal scalars crosses more than big_span chunks at every
    length (big list); six runs of exactly L equal scalars for each length L are cut exactly once at that length unless they start on a boundary (one in L, in each of
    the W windows), and the runs of 2 .. 60 are cut once or not at all at the longer lengths."""
    c, n = 17, N_OF[ZL_G2]
    B, S = _inputs(backend, g, n, 8300, c)
    at = _runs(S, 100, [8 * 128 + 128 + 5])
    at = _runs(S, at, [L for L in (8, 16, 32, 64, 128) for _ in range(6)])
    _runs(S, at, range(2, 61))
    with _case(backend, monkeypatch, g, B, S, c=c) as case:
        case.run({}, lambda p: p.chunk == 8 and p.by_cuts and p.big_span == 8 and p.may_big)
        for chunk in (16, 32, 64, 128):
            p = case.run({"CHUNK": chunk}, lambda p: p.chunk == chunk and p.by_cuts and p.big_span == 8 and p.may_big)
            assert 8 * 128 + 128 + 5 > p.big_span * p.chunk + p.chunk


# ------------------------------------------------------------------------------------------------ (c) big_span = 64
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_g1_big_span_64(backend, monkeypatch, curve):
    """c = 8 at n = 2^15 + 3 is more than 2^20 entries in 128 buckets per window: with 8-entry chunks nchunks > 2^17 and big_span is 64.  A uniform bucket holds 256
    entries (BLS12-381, on 2 n half-scalars: 512) -- 32 (64) chunks, folded serially here and on the big list at span 8; a run of 1500 equal scalars is cut into more
    than 64 chunks.  Once with the per-bucket merge (2048 / 4096 buckets), once with the merge by chunk boundaries on one lane."""
    g, c, n = (curve, ZL_G1), 8, N_MAX
    B, S = _inputs(backend, g, n, 8400, c)
    _runs(S, 100, [1500])
    with _case(backend, monkeypatch, g, B, S, c=c) as case:
        case.run({}, lambda p: p.big_span == 8 and p.nchunks <= 1 << 17)
        p = case.run({"CHUNK": 8}, lambda p: p.chunk == 8 and p.nchunks > 1 << 17 and p.big_span == 64 and not p.by_cuts and p.may_big and p.may_giant)
        per_bucket = n * p.endo_k // (1 << (c - 1))
        assert 8 * p.chunk < per_bucket <= 64 * p.chunk + p.chunk and 1500 > 64 * p.chunk + p.chunk
        case.run({"CHUNK": 8, "QUAD_LANES": 0}, lambda p: p.nchunks > 1 << 17 and p.big_span == 64 and p.by_cuts)


# ------------------------------------------------------------------------------------------------ (d) accumulation form
@pytest.mark.parametrize("g", GROUPS, ids=_gid)
def test_accumulation_forms(backend, monkeypatch, g):
    """the input of (a) under k_msm_accumulate_quad / _pair<true> (a threshold above nchunks) and k_msm_accumulate / _pair<false> (threshold 0): byte-equal"""
    c = 17
    B, S = _inputs(backend, g, N_OF[ZL_G2], 8500, c)
    _runs(S, _runs(S, 100, [200]), range(2, 61))
    with _case(backend, monkeypatch, g, B, S, c=c) as case:
        case.run({"QUAD_ACC_CHUNKS": 0}, lambda p: not p.acc_quad and p.nchunks > 1)
        case.run({"QUAD_ACC_CHUNKS": ABOVE_ALL}, lambda p: p.acc_quad and p.nchunks > 1)


# ------------------------------------------------------------------------------------------------ (e) tail forms
@pytest.mark.parametrize("g", GROUPS, ids=_gid)
@pytest.mark.parametrize("c", [9, 13, 0], ids=["c9", "c13", "table16"])
def test_tail_one_lane_on_few_buckets(backend, monkeypatch, g, c):
    """ZL_TUNE_QUAD_LANES = 0 on a few thousand buckets: the merge by chunk boundaries, and level 0 and every tree level on one lane (G2: a lane pair); byte-equal to the
    four- / eight-lane kernels of the default.  A tree level runs SETS * nodes * (level + 2) lanes: with the 8 .. 15 sets of c = 9 and c = 13 even the root level is two
    waves, so the levels BELOW one wave are met on the single set of a 16-bit table, whose three upper levels run 56, 30 and 16 lanes."""
    n = 3001 if g[1] == ZL_G1 else 1501
    B, S = _inputs(backend, g, n, 8600 + c, c or 16)
    _runs(S, _runs(S, 100, [200]), range(2, 41))
    with _case(backend, monkeypatch, g, B, S, c=c, table=0 if c else 16) as case:
        case.run({}, lambda p: not p.by_cuts and p.NB <= p.tail_quad_max)
        p = case.run({"QUAD_LANES": 0}, lambda p: p.by_cuts and p.tail_quad_max == 0 and p.nchunks > 1 and p.red_levels >= 6)
        assert (p.SETS * (p.red_levels + 2) < 32) == (c == 0) == bool(p.pre)


@pytest.mark.parametrize("g", GROUPS, ids=_gid)
def test_tail_quad_on_many_buckets(backend, monkeypatch, g):
    """a lane threshold above NB at c = 17: the per-bucket merge k_msm_merge<G, true> / k_msm_merge_pair<G, true> hands the cut buckets on, level 0 and the tree run on
    four / eight lanes at every level; byte-equal to the one-lane kernels of the default"""
    c = 17
    B, S = _inputs(backend, g, N_OF[ZL_G2], 8700, c)
    _runs(S, _runs(S, 100, [200]), range(2, 61))
    with _case(backend, monkeypatch, g, B, S, c=c) as case:
        case.run({}, lambda p: p.by_cuts and p.NB > p.tail_quad_max)
        case.run({"QUAD_LANES": ABOVE_ALL}, lambda p: not p.by_cuts and (1 << 16) < p.NB <= p.tail_quad_max and p.may_big)


@pytest.mark.parametrize("g", GROUPS, ids=_gid)
def test_tail_single_chunk_merge(backend, monkeypatch, g):
    """five scalars in one 128-entry chunk at c = 17: no chunk boundary, so the many buckets take the one-lane per-bucket merge, k_msm_merge<G> / k_msm_merge_pair<G, false>"""
    c, n = 17, 5
    B = _pts(backend, g)[:n]
    S = ol.random_scalars(g[0], n, 8800)
    S[1] = ol.ints_to_limbs([g[0].fr.p - 1], 4)[0]
    S[3] = S[2]
    with _case(backend, monkeypatch, g, B, S, c=c) as case:
        case.run({"CHUNK": 128}, lambda p: p.nchunks == 1 and p.NB > p.tail_quad_max and not p.by_cuts and not p.may_big)
        case.run({}, lambda p: p.nchunks > 1 and p.by_cuts)


# ------------------------------------------------------------------------------------------------ (f) red_g0
@pytest.mark.parametrize("g", GROUPS, ids=_gid)
def test_reduction_block_lengths(backend, monkeypatch, g):
    """ZL_TUNE_SEG 2 / 4 / 8 at windows of every kind, picked from the plan hook's spread_t at SEG = 8 among c = 2 .. 20 (the smallest and the largest window of each kind):
    a spread top window of 1 or 2 bits (level-0 blocks shortened to 2^spread_t), spread_t == 0 (level 0 weightless for that set), no spread, and H < 8 (g0 clamped)"""
    n = 1500
    B, S = _inputs(backend, g, n, 8900, 2)
    exp = _oracle(g, B, S)
    kinds = {"short": [], "zero": [], "none": [], "clamp": []}
    with _case(backend, monkeypatch, g, B, S, expect=False) as case:
        case.exp = exp
        for c in range(2, 21):
            case.c = c
            p = case.plan({"SEG": 8})
            H = 1 << (p.c - 1)
            assert p.c == c and p.red_g0 <= min(8, H)
            if H < 8:
                kinds["clamp"].append(c)
            elif 0 < p.spread_t < 3:
                kinds["short"].append(c)
            elif p.spread_t == 0:
                kinds["zero"].append(c)
            elif p.spread_t < 0:
                kinds["none"].append(c)
            if p.spread_t == 0 and c not in kinds["zero"]:
                kinds["zero"].append(c)
        assert all(kinds.values()), kinds
        for kind, cs in kinds.items():
            for c in sorted({cs[0], cs[-1]}):
                case.c, case.results = c, []
                for seg in (2, 4, 8):
                    p = case.run({"SEG": seg}, lambda p: p.red_g0 <= seg and p.red_levels == p.c - 1 - (p.red_g0.bit_length() - 1))
                    H = 1 << (c - 1)
                    if kind == "short":
                        assert p.red_g0 == min(seg, 1 << p.spread_t) and (seg < 8 or p.red_g0 < seg), (c, seg, p)
                    elif kind == "clamp":
                        assert p.red_g0 == min(seg, H) and (seg < 8 or p.red_g0 == H < seg), (c, seg, p)
                    elif kind == "none":
                        assert p.red_g0 == seg and p.spread_t == -1, (c, seg, p)
                    elif H >= 8:
                        assert p.red_g0 == seg and p.spread_t == 0, (c, seg, p)


# ------------------------------------------------------------------------------------------------ (g) LDS sort
@pytest.mark.parametrize("g", GROUPS, ids=_gid)
def test_lds_sort_prefix_and_ranges(backend, monkeypatch, g):
    """the windows with the most buckets at or below 14 336 (k_msm_prefix_small) and the fewest above (k_msm_slice_prefix and the three-kernel scan), found with the plan
    hook among c = 2 .. 16, and 1 / 4 / 64 scatter ranges at c = 13; n is no multiple of the recoder's 256 scalars nor of the slice count"""
    n = 3 * 4096 + 1 if g[1] == ZL_G1 else N_OF[ZL_G2]
    B, S = _inputs(backend, g, n, 9000, 13)
    _runs(S, 100, [300])
    with _case(backend, monkeypatch, g, B, S) as case:
        plans = {}
        for c in range(2, 17):
            case.c = c
            p = case.plan({})
            if p.sort_lds:
                plans[c] = (p.NB, bool(p.lds_prefix_small))
        below = max((c for c in plans if plans[c][1]), key=lambda c: plans[c][0])
        above = min((c for c in plans if not plans[c][1]), key=lambda c: plans[c][0])
        assert 12288 <= plans[below][0] <= 14336 < plans[above][0] <= 24576, plans
        ragged = lambda p: p.nslices > 1 and (n * p.endo_k) % 256 != 0 and (n * p.endo_k) % p.nslices != 0  # noqa: E731
        for c, small in ((below, True), (above, False)):
            case.c, case.results = c, []
            case.run({}, lambda p: p.sort_lds and bool(p.lds_prefix_small) == small and ragged(p))
        case.c, case.results = 13, []
        case.run({}, lambda p: p.sort_lds and ragged(p) and p.lds_ranges in (16, 32, 64))
        for ranges in (1, 4, 64):
            case.run({"RANGES": ranges}, lambda p: p.sort_lds and p.lds_ranges == ranges and (1 << 12) // ranges >= 64)


# ------------------------------------------------------------------------------------------------ (h) wide sort
def _sub_group_runs(S, at, c, windows):
    """1100 scalars whose only non-zero digit, in window w, lies in [257, 512): one 256-bucket sub-group of that window holds all of them"""
    for w in windows:
        vals = [(257 + (j % 255)) << (c * w) for j in range(1100)]
        S[at:at + 1100] = ol.ints_to_limbs(vals, 4)
        at += 1100
    return at


@pytest.mark.parametrize("g", GROUPS, ids=_gid)
@pytest.mark.parametrize("table", [0, 16], ids=["window", "table"])
def test_wide_sort_forms(backend, monkeypatch, g, table):
    """the three-level sort over plain 17-bit windows and over the merged set of a 16-bit table: k_msm_fine_sort on 256, 512 and 1024 threads, and with a stage of 1024
    entries two sub-groups of 1100 entries each (digits 257 .. 511 of windows 0 and 1; on the table they share one sub-group) go to k_msm_fine_sort_big's queue;
    several slices here, one slice below"""
    c, n = (0 if table else 17), N_OF[ZL_G2]
    B, S = _inputs(backend, g, n, 9100, 17)
    at = _sub_group_runs(S, 100, table or c, (0, 1))
    with _case(backend, monkeypatch, g, B, S, c=c, table=table) as case:
        p = case.run({}, lambda p: p.wide and bool(p.pre) == bool(table) and p.nslices > 1 and p.fine_threads == 1024 and p.fine_cap >= 4096 > 2 * 1100)
        if p.glv:
            _assert_first_part_only(backend, g, [257 << 17, 511 << 17, 257, 511])
        for fs in (256, 512):
            case.run({"FS": fs}, lambda p: p.wide and p.fine_threads == fs)
        case.run({"FS_CAP": 1024}, lambda p: p.wide and p.fine_cap == 1024 < 1100)
        case.run({"FS_CAP": 1024, "FS": 256}, lambda p: p.wide and p.fine_cap == 1024 and p.fine_threads == 256)
    n1 = 1000
    with _case(backend, monkeypatch, g, B[:n1], S[at:at + n1], c=c, table=table) as case:
        case.run({}, lambda p: p.wide and p.nslices == 1 and p.per_slice == n1 * p.endo_k)
        case.run({"FS": 256, "FS_CAP": 1024}, lambda p: p.wide and p.nslices == 1 and p.fine_threads == 256)


# ------------------------------------------------------------------------------------------------ (i) the batch driver at small n
def _batch_vectors(curve, n, seed):
    """scalar vectors that differ in where their cut buckets, scalar-1 lists and big buckets sit"""
    vecs = [ol.random_scalars(curve, n, seed + j) for j in range(6)]
    vecs[1][: n // 2] = ol.ints_to_limbs([1], 4)[0]
    _runs(vecs[2], n // 3, [300])
    _runs(vecs[3], 10, range(2, 40))
    vecs[4][n // 2:] = vecs[4][n // 2]
    _runs(vecs[5], n // 2, [100, 9, 17])
    return vecs


def _check_batch(backend, g, h, dev, order, single, exp0):
    import torch

    batch = backend.msm_batch_partial_dev(h, [dev[j].data_ptr() for j in order], dev[0].shape[0])
    torch.cuda.synchronize()
    for i, j in enumerate(order):
        a, ai = backend.partials_sum(g[0].cid, batch[i:i + 1], group=g[1])
        assert ai == single[j][1] and a.tobytes() == single[j][0].tobytes(), (order, i)
    if exp0 is not None:
        a, ai = backend.partials_sum(g[0].cid, batch[0:1], group=g[1])
        assert ai == exp0[1] and (a == exp0[0]).all()


def _flavours(g):
    """(name, n, table, knobs, glv): the sizes at which the planner keeps plain scalars exist on BN254 only (G1 from 2^13 on, G2 from 2^11 to below 2^17)"""
    out = [("split", 1500, 0, {}, True), ("split-own-phi", 1500, 0, {"ENDO_CACHE_MB": 0}, True), ("table", 1500, 16, {}, False)]
    if g[0] is po.BN254:
        out.append(("plain", N_OF[ZL_G2], 0, {}, False))
    return out


@pytest.mark.parametrize("g", GROUPS, ids=_gid)
def test_pipeline_small_batches(backend, monkeypatch, g):
    """ZL_TUNE_SIDE_BY_SIDE_LOG = 0: batches of 2, 3, 4 and 7 jobs on the three-stream pipeline over three rotating buffer sets (7: every set is reused twice), an all-zero
    vector in the middle; on split scalars with the images of the bases kept with the handle, on split scalars with the cache off (job 0 computes the images, the later
    jobs borrow them), on a table and, where the planner keeps them, on plain scalars.  Every partial equals the single call's, job 0 the oracle's; each batch runs twice."""
    import torch

    for name, n, table, extra, glv in _flavours(g):
        B = _pts(backend, g)[:n]
        vecs = _batch_vectors(g[0], n, 9200)
        zero = len(vecs)
        vecs.append(np.zeros((n, 4), dtype=np.uint64))
        dev = [torch.from_numpy(S.view(np.int64)).cuda() for S in vecs]
        torch.cuda.synchronize()
        exp0 = _oracle(g, B, vecs[0])
        h = backend.bases_upload(g[0].cid, np.ascontiguousarray(B), group=g[1])
        try:
            if table:
                backend.bases_precompute(h, table)
            with _env(monkeypatch, dict(extra, SIDE_BY_SIDE_LOG=0)):
                p = hook_msm_plan(backend, h, n)
                assert bool(p.glv) == glv and bool(p.pre) == bool(table), (name, p)
                single = [backend.partials_sum(g[0].cid, backend.msm_partial_dev(h, d.data_ptr(), n).reshape(1, -1), group=g[1]) for d in dev]
                assert single[zero][1] == 1
                for count in (2, 3, 4, 7):
                    form = hook_msm_batch_form(count, n)
                    assert not form["side"] and form["lanes"] == 3 and not form["phased"], form
                    order = list(range(count - 1)) if count < 7 else [0, 1, 2, 3, 4, 5]
                    order.insert(count // 2, zero)
                    assert len(order) == count
                    for rep in range(2):
                        _check_batch(backend, g, h, dev, order, single, exp0 if order[0] == 0 else None)
        finally:
            backend.bases_free(h)


@pytest.mark.parametrize("g", GROUPS, ids=_gid)
def test_side_by_side_lanes_and_phases(backend, monkeypatch, g):
    """the other form of the same decision: side-by-side lanes, four jobs on 1, 2, 3 and 4 lanes (a lane's buffer set is reused by the job behind it), and the phase-major
    issue order (all sorts, then accumulations and tails) that the default keeps for jobs of 2^17 points and more"""
    import torch

    n = 1500
    B = _pts(backend, g)[:n]
    vecs = _batch_vectors(g[0], n, 9300)[:3] + [np.zeros((n, 4), dtype=np.uint64)]
    dev = [torch.from_numpy(S.view(np.int64)).cuda() for S in vecs]
    torch.cuda.synchronize()
    exp0 = _oracle(g, B, vecs[0])
    h = backend.bases_upload(g[0].cid, np.ascontiguousarray(B), group=g[1])
    try:
        with _env(monkeypatch, {}):
            single = [backend.partials_sum(g[0].cid, backend.msm_partial_dev(h, d.data_ptr(), n).reshape(1, -1), group=g[1]) for d in dev]
        order = [0, 1, 3, 2]
        for knobs, lanes, phased in (({}, 4, False), ({"SIDE_LANES": 1}, 1, False), ({"SIDE_LANES": 2}, 2, False), ({"SIDE_LANES": 3}, 3, False),
                                     ({"PHASED_MIN_LOG": 0}, 4, True), ({"PHASED_MIN_LOG": 0, "SIDE_LANES": 3}, 3, False)):
            with _env(monkeypatch, knobs):
                form = hook_msm_batch_form(len(order), n)
                assert form == {"side": True, "lanes": lanes, "phased": phased}, (knobs, form)
                for rep in range(2):
                    _check_batch(backend, g, h, dev, order, single, exp0)
    finally:
        backend.bases_free(h)


# ------------------------------------------------------------------------------------------------ (j) heterogeneous jobs on the pipeline
@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_groth16_proof_on_the_pipeline(backend, monkeypatch, curve):
    """one proof of the one-hash Poseidon circuit with its MSMs on the three-stream pipeline -- a batch that is not over one key: the proof equals the knob-free proof
    byte for byte.  A proof this small folds its G1 work into two jobs (the a query, and one query for all of C); with ZL_TUNE_G16_FOLD_LOG_N = 0 it runs the four G1
    MSMs of a large proof, which differ in handle and n, so that the fourth job waits for the buffer set of the first; the G2 MSM is a single call beside them.  With
    the images of the bases kept with the handles and (a fresh key) with one image per buffer set."""
    circ = Circuit(curve.cid, 1)
    keys = [Groth16Keys(backend, circ, seed=0x9E0) for _ in range(2)]
    same = lambda p, q: all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(p, q))  # noqa: E731
    try:
        with _env(monkeypatch, {}):
            assert hook_msm_batch_form(4, 1 << 10)["side"]
            ref, _, _ = keys[0].prove(seed=5)
            assert keys[0].verify(ref, circ.arrays()["assignment"][1:2])
        for k, knobs in ((keys[0], {"SIDE_BY_SIDE_LOG": 0}), (keys[0], {"SIDE_BY_SIDE_LOG": 0, "G16_FOLD_LOG_N": 0}), (keys[0], {"G16_FOLD_LOG_N": 0}),
                         (keys[1], {"SIDE_BY_SIDE_LOG": 0, "G16_FOLD_LOG_N": 0, "ENDO_CACHE_MB": 0})):
            with _env(monkeypatch, knobs):
                form = hook_msm_batch_form(4, 1 << 10)
                assert form["side"] == ("SIDE_BY_SIDE_LOG" not in knobs) and (form["side"] or form["lanes"] == 3)
                for rep in range(2):
                    got, _, _ = k.prove(seed=5)
                    assert same(got, ref), (knobs, rep)
    finally:
        for k in keys:
            k.close()
        circ.close()


# ------------------------------------------------------------------------------------------------ (k) batched inversion
@pytest.mark.parametrize("g", GROUPS, ids=_gid)
def test_batch_inversion_lengths(backend, monkeypatch, g):
    """bases_generate and the download of 1000 points with 1, 7 and 64 points per batched inversion (and the default), against the oracle's k_i G"""
    curve, n = g[0], 1000
    k = ol.random_scalars(curve, n, 9400)
    k[3] = ol.ints_to_limbs([1], 4)[0]
    k[4] = ol.ints_to_limbs([curve.fr.p - 1], 4)[0]
    k[6] = k[5]
    exp = ol.oracle_g1_mul_gen(curve, k) if g[1] == ZL_G1 else gu.g2_mul_gen(curve, ol.limbs_to_ints(k))
    for knobs in ({}, {"BATCH_INV": 1}, {"BATCH_INV": 7}, {"BATCH_INV": 64}):
        with _env(monkeypatch, knobs):
            h = backend.bases_generate(curve.cid, k, group=g[1])
            try:
                got = backend.bases_download(h)
                part = backend.bases_download(h, 3, 130)
            finally:
                backend.bases_free(h)
        assert (got == exp).all() and (part == exp[3:133]).all(), knobs

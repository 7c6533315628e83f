"""Poseidon at arities 3, 4, 5 (widths 4, 5, 6) on the device (csrc/zl_poseidon_dev.hip: k_pos_permute_w, k_pos_hash_w) against the Python model of
tests/poseidon_arity_util.py, at the smallest shapes that reach every branch: wave and block edges, several chunks, device pointers, the host path, a forked
lane, a foreign stream.  Every batch carries the BOUND cases -- all r - 1, all 0, r - 1 in exactly one position, the hash of `arity` copies of r - 1 -- which
drive the lazily reduced sums of the kernels to their largest values: where a weak reduction is missing they give a wrong digest, not a fault."""
import json
import os

import numpy as np
import pytest

import poseidon_arity_util as pa
import poseidon_util as pu
from oracle_lib import po
from openzl_amd import backend as zb

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FX = json.load(open(os.path.join(HERE, "golden", "ref_poseidon_fixtures.json")))
CURVES = pytest.mark.parametrize("curve", pa.CURVES, ids=lambda c: c.name)
WIDE = pytest.mark.parametrize("width", [4, 5, 6])
EINVAL = -1
HUGE = str(1 << 30)
N_RANDOM = 65


@pytest.fixture(autouse=True)
def device_path(monkeypatch):
    """every host-pointer call of this file runs on the device unless a test says otherwise"""
    monkeypatch.setenv("ZL_TUNE_POSEIDON_DEV_MIN", "0")


_REF = {}


def ref(curve, width):
    """(states, their permutations, the hashes of states[i][1:], the indices of the bound cases): the edge states of pa.edge_states -- the bound cases are its
    last width + 2 -- then 65 random ones; computed once per (curve, width) and shared, never changed"""
    key = (curve.name, width)
    if key not in _REF:
        states = pa.edge_states(curve, width)
        n_edge = len(states)
        vals = pu.random_elems(curve, width * N_RANDOM, 100 + width)
        states += [vals[width * i:width * (i + 1)] for i in range(N_RANDOM)]
        bound = list(range(n_edge - width - 2, n_edge))
        _REF[key] = (states, [pa.permute(curve, s) for s in states], [pa.hash(curve, s[1:]) for s in states], bound)
    return _REF[key]


def selection(curve, width, count):
    """indices of a batch of `count` items: the bound cases first, the others in turn, and a bound case in the LAST lane again"""
    states, _, _, bound = ref(curve, width)
    others = [i for i in range(len(states)) if i not in bound]
    sel = (bound + [others[i % len(others)] for i in range(count)])[:count]
    if count > len(bound):
        sel[-1] = bound[0]  # all r - 1
    return sel


def words(states, sel, lo=0):
    """(len(sel), W - lo, 4) words of states[i][lo:]"""
    w = len(states[0]) - lo
    return pu.limbs([v for i in sel for v in states[i][lo:]]).reshape(len(sel), w, 4)


def dev(a: np.ndarray):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def host(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def hash_dev(backend, curve, arity, xs: np.ndarray) -> np.ndarray:
    n = xs.shape[0]
    d_in, d_out = dev(xs), dev(np.zeros((n, 4), dtype=np.uint64))
    backend.poseidon_hash_dev(curve.cid, arity, d_in.data_ptr(), n, d_out.data_ptr())
    return host(d_out).reshape(n, 4)


# ---- wave and block edges, with the bound cases -------------------------------------------------------------------------------------------------------
@CURVES
@WIDE
def test_permute_and_hash_at_wave_and_block_edges(backend, curve, width):
    states, exp_p, exp_h, bound = ref(curve, width)
    r = curve.fr.p
    assert states[bound[0]] == [r - 1] * width and states[bound[1]] == [0] * width
    assert [states[i] for i in bound[2:]] == [[r - 1 if j == pos else 0 for j in range(width)] for pos in range(width)]
    for i in bound:  # a batch of ONE: every bound case alone
        assert [pu.ints(g) for g in backend.poseidon_permute_batch(curve.cid, words(states, [i]))] == [exp_p[i]], i
        assert pu.ints(backend.poseidon_hash(curve.cid, words(states, [i], 1))) == [exp_h[i]], i
    for count in (1, 63, 64, 65, 257):
        sel = selection(curve, width, count)
        assert count == 1 or set(bound) <= set(sel)
        got = backend.poseidon_permute_batch(curve.cid, words(states, sel))
        assert got.shape == (count, width, 4) and [pu.ints(g) for g in got] == [exp_p[i] for i in sel], count
        got = backend.poseidon_hash(curve.cid, words(states, sel, 1))
        assert got.shape == (count, 4) and pu.ints(got) == [exp_h[i] for i in sel], count
    assert backend.poseidon_hash(curve.cid, np.zeros((0, width - 1, 4), dtype=np.uint64)).shape == (0, 4)
    assert backend.poseidon_permute_batch(curve.cid, np.zeros((0, width, 4), dtype=np.uint64)).shape == (0, width, 4)


@CURVES
@WIDE
def test_three_chunks_the_last_with_one_item(backend, curve, width, monkeypatch):
    monkeypatch.setenv("ZL_TUNE_POSEIDON_CHUNK", "256")
    states, exp_p, exp_h, _ = ref(curve, width)
    sel = selection(curve, width, 513)
    got = backend.poseidon_permute_batch(curve.cid, words(states, sel))
    assert [pu.ints(g) for g in got] == [exp_p[i] for i in sel]
    xs = words(states, sel, 1)
    got = backend.poseidon_hash(curve.cid, xs)
    assert pu.ints(got) == [exp_h[i] for i in sel]
    assert np.array_equal(hash_dev(backend, curve, width - 1, xs), got)


@CURVES
@WIDE
def test_device_device_pointer_and_host_paths_agree_byte_for_byte(backend, curve, width, monkeypatch):
    states, exp_p, exp_h, _ = ref(curve, width)
    sel = selection(curve, width, 300)
    xs, st = words(states, sel, 1), words(states, sel)
    on_dev = backend.poseidon_hash(curve.cid, xs)
    perm_dev = backend.poseidon_permute_batch(curve.cid, st)
    on_ptr = hash_dev(backend, curve, width - 1, xs)
    monkeypatch.setenv("ZL_TUNE_POSEIDON_DEV_MIN", HUGE)
    on_host = backend.poseidon_hash(curve.cid, xs)
    perm_host = backend.poseidon_permute_batch(curve.cid, st)
    assert on_dev.tobytes() == on_ptr.tobytes() == on_host.tobytes() == zb.poseidon_hash_host(curve.cid, xs).tobytes()
    assert perm_dev.tobytes() == perm_host.tobytes()
    assert pu.ints(on_dev) == [exp_h[i] for i in sel]


# ---- width 3 / arity 2 through the new entry points ---------------------------------------------------------------------------------------------------
@CURVES
def test_width_3_through_the_new_entry_points_is_the_width_3_unit(backend, curve):
    vals = pu.random_elems(curve, 3 * 65, 17) + [curve.fr.p - 1] * 3
    st = pu.limbs(vals).reshape(66, 3, 4)
    exp = backend.poseidon_permute_batch(curve.cid, st)
    got = st.copy()
    backend._check(backend.L.zl_poseidon_permute_batch_w(backend._ctx, curve.cid, 3, zb._p64(got), 66), "zl_poseidon_permute_batch_w")
    assert got.tobytes() == exp.tobytes()
    xy = np.ascontiguousarray(st[:, 1:, :])
    exp_h = backend.poseidon_hash2(curve.cid, xy)
    assert backend.poseidon_hash(curve.cid, xy).tobytes() == exp_h.tobytes() == hash_dev(backend, curve, 2, xy).tobytes()
    assert pu.ints(exp_h)[:2] == [pu.hash2(curve, *vals[1:3]), pu.hash2(curve, *vals[4:6])]


def test_h_1_2_through_the_new_entry_points_is_the_reference_digest(backend):
    cid = po.BLS12_381.cid
    assert str(pu.ints(backend.poseidon_hash(cid, pu.limbs([1, 2]).reshape(1, 2, 4)))[0]) == FX["permutation_width3"]["output"][0]
    st = pu.limbs([3, 1, 2]).reshape(1, 3, 4).copy()
    backend._check(backend.L.zl_poseidon_permute_batch_w(backend._ctx, cid, 3, zb._p64(st), 1), "zl_poseidon_permute_batch_w")
    assert [str(v) for v in pu.ints(st[0])] == FX["permutation_width3"]["output"]


# ---- non-canonical input ------------------------------------------------------------------------------------------------------------------------------
@CURVES
@pytest.mark.parametrize("width", pa.WIDTHS)
def test_non_canonical_input_is_refused(backend, curve, width):
    r, arity = curve.fr.p, width - 1
    base = pu.random_elems(curve, width * 65, 7)
    for at in (0, width * 65 - 1):
        vals = list(base)
        vals[at] = r
        with pytest.raises(zb.BackendError) as e:
            backend.poseidon_permute_batch(curve.cid, pu.limbs(vals).reshape(65, width, 4))
        assert e.value.code == EINVAL
    for at in (0, arity * 65 - 1):
        vals = list(base[:arity * 65])
        vals[at] = r
        xs = pu.limbs(vals).reshape(65, arity, 4)
        with pytest.raises(zb.BackendError) as e:
            backend.poseidon_hash(curve.cid, xs)
        assert e.value.code == EINVAL
        with pytest.raises(zb.BackendError) as e:
            hash_dev(backend, curve, arity, xs)
        assert e.value.code == EINVAL
    assert backend.poseidon_hash(curve.cid, pu.limbs(base[:arity * 65]).reshape(65, arity, 4)).shape == (65, 4)  # the flag does not stick


# ---- lanes and streams --------------------------------------------------------------------------------------------------------------------------------
@CURVES
def test_forked_lane_and_foreign_stream(backend, curve):
    import torch

    width = 5
    states, exp_p, exp_h, _ = ref(curve, width)
    sel = selection(curve, width, 65)
    xs, st = words(states, sel, 1), words(states, sel)
    root_h, root_p = backend.poseidon_hash(curve.cid, xs), backend.poseidon_permute_batch(curve.cid, st)
    assert pu.ints(root_h) == [exp_h[i] for i in sel]
    lane = backend.fork()
    try:
        assert lane.poseidon_hash(curve.cid, xs).tobytes() == root_h.tobytes()
        assert lane.poseidon_permute_batch(curve.cid, st).tobytes() == root_p.tobytes()
    finally:
        lane.close()
        backend._forks.remove(lane)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        backend.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            d_in = torch.from_numpy(xs.view(np.int64).copy()).cuda(non_blocking=False)
            d_out = torch.zeros(65 * 4, dtype=torch.int64, device="cuda")
            backend.poseidon_hash_dev(curve.cid, width - 1, d_in.data_ptr(), 65, d_out.data_ptr())
            assert host(d_out).reshape(65, 4).tobytes() == root_h.tobytes()
            assert backend.poseidon_permute_batch(curve.cid, st).tobytes() == root_p.tobytes()
        finally:
            backend.set_stream(0)

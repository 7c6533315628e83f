"""CPU tests of the NTT driver's pass plan (zl_ntt.hip: ntt_plan, through the zl_test_ntt_plan hook) and of the size lists of the GPU plan tests.

The plan decides which code a transform size reaches: the number of passes, odd pass sizes (a half round after the two-stage rounds), pass sizes above 8,
row tables or per-tile row twiddles.  tests/test_gpu_ntt_plans.py compares the kernel with the oracle at sizes chosen from this table; a change to the plan
fails here and tells its author to extend the GPU lists."""
import numpy as np
import pytest

import oracle_lib as ol
from oracle_lib import po
from openzl_amd.backend import BackendError, hook_ntt_plan

# an independent restatement of the plan for multi-pass sizes
PLAN_TABLE = {
    11: [6, 5], 12: [6, 6], 13: [6, 7], 14: [8, 6], 15: [8, 7], 16: [8, 8], 17: [6, 6, 5], 18: [6, 6, 6], 19: [6, 6, 7], 20: [8, 6, 6], 21: [8, 6, 7],
    22: [8, 8, 6], 23: [8, 8, 7], 24: [8, 8, 8], 25: [6, 6, 6, 7], 26: [8, 6, 6, 6], 27: [8, 6, 6, 7], 28: [8, 8, 6, 6], 29: [8, 8, 6, 7], 30: [8, 8, 8, 6],
    31: [8, 8, 8, 7], 32: [8, 8, 8, 8],
}


@pytest.mark.parametrize("log_n", range(33))
def test_plan_shape_and_table(log_n):
    sizes = hook_ntt_plan(log_n)
    assert sum(sizes) == log_n
    assert (len(sizes) == 1) == (log_n <= 10)
    assert 1 <= len(sizes) <= 4
    if log_n > 0:
        assert all(1 <= s <= 10 for s in sizes), sizes
    else:
        assert sizes == [0]
    if log_n <= 10:
        assert sizes == [log_n]
    else:
        assert sizes == PLAN_TABLE[log_n], "the plan changed: extend the size lists of tests/test_gpu_ntt_plans.py to the new pass sizes"


def test_plan_hook_rejects_bad_arguments():
    from openzl_amd.backend import load_library

    with pytest.raises(BackendError):
        hook_ntt_plan(33)
    assert load_library().zl_test_ntt_plan(5, None, None) == -1
    assert load_library().zl_test_ntt_fit_beside(None, 1) == -1


def test_gpu_size_lists_cover_every_plan():
    """every distinct tuple of pass sizes up to 2^28 is compared with a reference by some GPU test: with the oracle up to 2^26, device-resident above"""
    import test_gpu_ntt_plans as tp

    oracle_sizes = set(tp.BASE_SIZES) | set(tp.ORACLE_SIZES) | set(tp.REDUCED_VARIANTS)
    assert oracle_sizes == set(range(27)), sorted(set(range(27)) - oracle_sizes)
    assert not set(tp.BASE_SIZES) & set(tp.ORACLE_SIZES)
    device_sizes = {log_n for log_n, _ in tp.DEVICE_CASES}
    covered = {tuple(hook_ntt_plan(n)) for n in oracle_sizes | device_sizes}
    assert covered == {tuple(hook_ntt_plan(n)) for n in range(29)}
    # the reduced sizes: both curves at each, every variant at least once per curve across them
    for curve in tp.CURVES:
        seen = set()
        for log_n, variants in tp.REDUCED_VARIANTS.items():
            assert variants[curve.name]
            seen |= set(variants[curve.name])
        assert seen == set(tp.VARIANTS)
    # the device-resident sizes stay within each curve's two-adicity and reach the last size the driver plans differently
    for log_n, curve in tp.DEVICE_CASES:
        assert log_n <= curve.two_adicity
    assert device_sizes == {27, 28}


@pytest.mark.parametrize("curve", [po.BLS12_381, po.BN254], ids=lambda c: c.name)
def test_threaded_oracle_on_canonical_limbs_equals_canonical_oracle(curve):
    """The GPU plan tests feed canonical limbs to the threaded oracle entry, whose contract is Montgomery in / out.  The transform is linear, so the words
    x read as Montgomery forms (of x / R) come back as NTT(x / R) R = NTT(x): pinned here against the single-threaded canonical entry and the explicit
    conversion, all four variants."""
    fid = 2 if curve.cid == 1 else 4
    for log_n in (3, 12):
        x = ol.random_scalars(curve, 1 << log_n, 31 + log_n)
        for inverse, coset in [(False, False), (True, False), (False, True), (True, True)]:
            exp = ol.oracle_ntt(curve, x, inverse=inverse, coset=coset, mont=False)
            got, _ = ol.oracle_ntt_timed(curve, x, inverse=inverse, coset=coset, threads=4)
            assert (got == exp).all()
            xm = np.zeros_like(x)
            ol.lib().zlo_field_to_mont(fid, ol.p64(x.reshape(-1)), ol.p64(xm.reshape(-1)), x.shape[0])
            gm, _ = ol.oracle_ntt_timed(curve, xm, inverse=inverse, coset=coset, threads=4)
            back = np.zeros_like(x)
            ol.lib().zlo_field_from_mont(fid, ol.p64(gm.reshape(-1)), ol.p64(back.reshape(-1)), x.shape[0])
            assert (back == exp).all()

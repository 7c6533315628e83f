"""Three staged loops of csrc/zl_poseidon_dev.hip crossed at a chunk boundary, both curves: zl_poseidon_chain_batch (host operands, three segments), the
device-pointer hash at every arity (no segment: the launch chunk alone) and the device-pointer duplex cipher (no segment encrypting, the verdicts' segment
decrypting).  ZL_TUNE_POSEIDON_CHUNK is set so that the last chunk is a partial one; the expectation is the host path of the same entry point, which the other
Poseidon tests pin to the Python model and the reference's fixtures."""
import numpy as np
import pytest

import poseidon_arity_util as pa
import poseidon_duplex_util as du
import poseidon_util as pu
from openzl_amd import backend as zb

pytestmark = pytest.mark.gpu

CURVES = pytest.mark.parametrize("curve", pa.CURVES, ids=lambda c: c.name)
EINVAL = -1


@pytest.fixture(autouse=True)
def device_path(monkeypatch):
    monkeypatch.setenv("ZL_TUNE_POSEIDON_DEV_MIN", "0")


def dev(a: np.ndarray):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    return t


def host(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


@CURVES
def test_chain_over_three_chunks_and_a_flag_that_does_not_stick(backend, curve, monkeypatch):
    monkeypatch.setenv("ZL_TUNE_POSEIDON_CHUNK", "48")
    count, k = 130, 2  # 48 + 48 + 34
    x0, x1 = pu.limbs(pu.random_elems(curve, count, 41)), pu.limbs(pu.random_elems(curve, count, 42))
    want = zb.poseidon_chain_host(curve.cid, x0, x1, k)
    assert backend.poseidon_chain(curve.cid, x0, x1, k).tobytes() == want.tobytes()
    bad = x1.copy()
    bad[70] = pu.limbs([curve.fr.p])[0]  # in the second chunk
    with pytest.raises(zb.BackendError) as e:
        backend.poseidon_chain(curve.cid, x0, bad, k)
    assert e.value.code == EINVAL
    assert backend.poseidon_chain(curve.cid, x0, x1, k).tobytes() == want.tobytes()


@CURVES
@pytest.mark.parametrize("arity", pa.ARITIES)
def test_hash_dev_over_three_chunks_writes_nothing_behind_its_rows(backend, curve, arity, monkeypatch):
    monkeypatch.setenv("ZL_TUNE_POSEIDON_CHUNK", "32")
    count = 65  # 32 + 32 + 1
    inputs = pu.limbs(pu.random_elems(curve, count * arity, 50 + arity)).reshape(count, arity, 4)
    want = zb.poseidon_hash_host(curve.cid, inputs)
    sentinel = np.uint64(0xA5A5A5A5A5A5A5A5)
    d_in, d_out = dev(inputs), dev(np.full((count + 1, 4), sentinel, dtype=np.uint64))
    backend.poseidon_hash_dev(curve.cid, arity, d_in.data_ptr(), count, d_out.data_ptr())
    out = host(d_out).reshape(count + 1, 4)
    assert out[:count].tobytes() == want.tobytes()
    assert (out[count] == sentinel).all()


@CURVES
@pytest.mark.parametrize("width", [3, 6])
def test_duplex_dev_over_three_chunks_and_one_wrong_tag(backend, curve, width, monkeypatch):
    monkeypatch.setenv("ZL_TUNE_POSEIDON_CHUNK", "32")
    count, shape = 65, (2, 1, 2)  # 32 + 32 + 1 messages of key 2, header 1, 2 blocks
    st = pu.limbs(pu.random_elems(curve, width, 60 + width))
    keys, headers, texts = du.pack(du.random_items(curve, width, shape, count, 70 + width), width, shape)
    want_ct, want_tags = zb.poseidon_duplex_encrypt_host(curve.cid, st, keys, headers, texts)
    d_k, d_h, d_t = dev(keys), dev(headers), dev(texts)
    d_ct, d_tags = dev(np.zeros_like(texts)), dev(np.zeros((count, 4), dtype=np.uint64))
    backend.poseidon_duplex_encrypt_dev(curve.cid, width, st, d_k.data_ptr(), 2, d_h.data_ptr(), 1, d_t.data_ptr(), 2, count, d_ct.data_ptr(), d_tags.data_ptr())
    assert host(d_ct).tobytes() == want_ct.tobytes() and host(d_tags).tobytes() == want_tags.tobytes()

    d_back = dev(np.zeros_like(texts))
    ok = backend.poseidon_duplex_decrypt_dev(curve.cid, width, st, d_k.data_ptr(), 2, d_h.data_ptr(), 1, d_ct.data_ptr(), d_tags.data_ptr(), 2, count, d_back.data_ptr())
    assert ok.shape == (count,) and ok.all() and host(d_back).tobytes() == texts.tobytes()

    bad = want_tags.copy()
    bad[40, 0] ^= np.uint64(1)  # in the second chunk
    d_bad, d_back = dev(bad), dev(np.zeros_like(texts))
    ok = backend.poseidon_duplex_decrypt_dev(curve.cid, width, st, d_k.data_ptr(), 2, d_h.data_ptr(), 1, d_ct.data_ptr(), d_bad.data_ptr(), 2, count, d_back.data_ptr())
    assert [i for i in range(count) if not ok[i]] == [40] and host(d_back).tobytes() == texts.tobytes()

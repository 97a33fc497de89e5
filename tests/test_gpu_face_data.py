"""csrc/face_batch.hip on the GPU: every tensor of a batch must equal FaceStore.host_batch -- the reference's arithmetic, which
tests/test_face_data_cpu.py holds against the reference itself -- bit for bit.  Destinations are handed in prefilled (NaN, or a
sentinel for the integer ones) with guard cells on both sides that must come back untouched."""
import itertools

import numpy as np
import pytest
import torch

import face_data_cases as fc
from ffwm_amd import data as fd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENTINEL = {torch.float32: float("nan"), torch.int64: -7777, torch.int32: -7}
_STORES = {}


def _stores(H, W, L):
    """(host store, device store) of 3 identities = 6 pairs = 12 items, built once per shape."""
    if (H, W, L) not in _STORES:
        c = fc.synthetic(3, H, W, L, seed=H * 1000 + W + L)
        host = fd.FaceStore.from_arrays(c["images"], c["masks"], c["names"], c["lm_dicts"])
        _STORES[(H, W, L)] = (host, host.to(DEV), {})
    return _STORES[(H, W, L)]


def _want(H, W, L, indices):
    host, _, cache = _stores(H, W, L)
    if tuple(indices) not in cache:
        w = host.host_batch(indices)
        del w["input_path"]
        cache[tuple(indices)] = w
    return cache[tuple(indices)]


def _guarded(B, H, W, L, keys):
    shapes = {"img_S": ((B, 3, H, W), torch.float32), "img_F": ((B, 3, H, W), torch.float32), "mask_S": ((B, 1, H, W), torch.float32),
              "mask_F": ((B, 1, H, W), torch.float32), "lm_S": ((B, L, 2), torch.int64), "lm_F": ((B, L, 2), torch.int64),
              "gate": ((B, L, 1), torch.float32), "invalid": ((B,), torch.int32)}
    flats, out = {}, {}
    for k in keys:
        shape, dt = shapes[k]
        n = int(np.prod(shape))
        flats[k] = torch.full((n + 2 * GUARD,), SENTINEL[dt], dtype=dt, device=DEV)
        out[k] = flats[k][GUARD:GUARD + n].view(shape)
    return flats, out


def _guards_untouched(flats, out):
    for k, f in flats.items():
        first = out[k].storage_offset()
        g = torch.cat((f[:first], f[first + out[k].numel():]))
        assert g.numel() >= 2 * GUARD
        assert bool(torch.isnan(g).all()) if f.dtype == torch.float32 else bool((g == SENTINEL[f.dtype]).all()), k


def _index(indices):
    return torch.tensor(indices, dtype=torch.int64).to(torch.int32).to(DEV)


INDICES = {1: [8], 8: [0, 7, 3, 11, 3, 6, 5, 9]}          # flipped (>= 6) and unflipped, 3 twice


@pytest.mark.parametrize("hw,B,L", list(itertools.product([(128, 128), (16, 16), (5, 7)], [1, 8], [1, 580, 1024])))
def test_batch_equals_host_batch(hw, B, L):
    H, W = hw
    _, dev, _ = _stores(H, W, L)
    flats, out = _guarded(B, H, W, L, fd.TRAIN_KEYS + ("invalid",))
    res = dev.batch(_index(INDICES[B]), out=out)
    want = _want(H, W, L, INDICES[B])
    assert set(res) == set(want) | {"invalid"} and len(want) == 7
    for k, w in want.items():
        assert res[k] is out[k] and res[k].dtype == w.dtype and torch.equal(res[k].cpu(), w), k
    assert res["invalid"].tolist() == [0] * B
    _guards_untouched(flats, out)


def test_every_byte_value_and_fractional_landmarks():
    """The s16 set of the CPU fixture (image 0 holds every byte value; landmarks non-integral and out of range), all 10 items."""
    c = fc.case("s16")
    host = fd.FaceStore.from_arrays(c["images"], c["masks"], c["names"], c["lm_dicts"], load_size=16)
    idx = list(range(len(host)))
    res, want = host.to(DEV).batch(_index(idx)), host.host_batch(idx)
    assert res["img_S"][0].unique().numel() == 256
    for k in fd.TRAIN_KEYS:
        assert torch.equal(res[k].cpu(), want[k]), k


def test_out_of_range_indices_give_zeros_and_a_flag():
    H, W, L = 5, 7, 580
    _, dev, _ = _stores(H, W, L)
    bad = [-1, 2, 12, 9, -2 ** 31, 2 ** 31 - 1]          # 2 P = 12
    flats, out = _guarded(len(bad), H, W, L, fd.TRAIN_KEYS + ("invalid",))
    res = dev.batch(_index(bad), out=out)
    assert res["invalid"].tolist() == [1, 0, 1, 0, 1, 1]
    want = _want(H, W, L, [2, 9])
    for k in fd.TRAIN_KEYS:
        got = res[k].cpu()
        assert torch.equal(got[[1, 3]], want[k]), k                                     # the neighbours are served
        assert bool((got[[0, 2, 4, 5]] == 0).all()), k                                  # (NaN prefill: a cell left unwritten is not 0)
    _guards_untouched(flats, out)


def test_test_batches():
    c = fc.synthetic(3, 16, 16, 1, seed=5)
    host = fd.FaceStore.from_arrays(c["images"], None, c["names"], isval=True)
    dev = host.to(DEV)
    idx = [5, 0, 0, 6, -1]          # P = 6: item 6 does not exist in a test set
    flats, out = _guarded(len(idx), 16, 16, 1, fd.TEST_KEYS + ("invalid",))
    res = dev.batch(_index(idx), out=out)
    want = host.host_batch(idx[:3])
    assert set(res) == {"img_S", "img_F", "invalid"} and res["invalid"].tolist() == [0, 0, 0, 1, 1]
    for k in fd.TEST_KEYS:
        assert torch.equal(res[k][:3].cpu(), want[k]) and bool((res[k][3:] == 0).all()), k
    _guards_untouched(flats, out)


def test_loader_epoch_and_its_buffers():
    H, W, L = 16, 16, 580
    host, dev, _ = _stores(H, W, L)
    loader = fd.FaceLoader(dev, 5, seed=3)
    batches = []
    for b in loader:
        batches.append((b, {k: v.cpu() for k, v in b.items()}))          # (read before the batch after next overwrites it)
    order = loader.permutation(0).tolist()
    assert sorted(order) == list(range(12)) and [b.batch_weight for b, _ in batches] == [5, 5, 2]
    for s, (b, got) in enumerate(batches):
        want = host.host_batch(order[5 * s:5 * s + 5])
        assert b.input_path == want.pop("input_path") and set(got) == set(want) == set(fd.TRAIN_KEYS)
        assert all(torch.equal(got[k], want[k]) for k in want)
    # two buffer sets, used alternately
    ptrs = [b["img_S"].data_ptr() for b, _ in batches]
    assert ptrs[0] != ptrs[1] and ptrs[2] == ptrs[0]
    assert torch.cat([b.invalid for b, _ in batches]).tolist() == [0] * 12


def test_out_is_written_in_place():
    from ffwm_amd.trainer import synthetic_batch
    H, W, L = 128, 128, 1024
    host, dev, _ = _stores(H, W, L)
    static = synthetic_batch(4, DEV)          # a trainer's static inputs have this form
    ptrs = {k: v.data_ptr() for k, v in static.items()}
    loader = fd.FaceLoader(dev, 4, seed=1, drop_last=True, out=static)
    order = loader.permutation(0).tolist()
    for s, b in enumerate(loader):
        assert set(b) == set(static) and all(b[k] is static[k] and b[k].data_ptr() == ptrs[k] for k in static)
        want = _want(H, W, L, order[4 * s:4 * s + 4])
        assert all(torch.equal(static[k].cpu(), want[k]) for k in static)
    assert set(static) == set(fd.TRAIN_KEYS)          # the caller's dict is left as it was


def test_a_captured_launch_follows_the_index_tensor():
    from ffwm_amd import graphs
    H, W, L = 16, 16, 580
    _, dev, _ = _stores(H, W, L)
    first, second = [0, 7, 3, 11], [10, 1, 1, 4]
    index = _index(first)
    _, out = _guarded(4, H, W, L, fd.TRAIN_KEYS + ("invalid",))
    graphs.warm_up(lambda: dev.batch(index, out=out), 2, sync=True)
    g, _ = graphs.capture(lambda: dev.batch(index, out=out))
    g.replay()
    for k, w in _want(H, W, L, first).items():
        assert torch.equal(out[k].cpu(), w), k
    index.copy_(_index(second))
    g.replay()
    for k, w in _want(H, W, L, second).items():
        assert torch.equal(out[k].cpu(), w), k


def test_gallery_planes_equal_the_host():
    for c, load in ((fc.case("s16"), 16), (fc.synthetic(3, 5, 7, 1, seed=9), 128), (fc.synthetic(2, 128, 128, 1, seed=10), 128)):
        host = fd.FaceStore.from_arrays(c["images"], None, c["names"], isval=True, load_size=load)
        ids, planes = host.to(DEV).gallery()
        want_ids, want = host.host_gallery()
        assert ids == want_ids and len(ids) >= 2 and planes.dtype == torch.float32 and torch.equal(planes.cpu(), want)

"""ffwm_face_batch_aug (csrc/face_batch.hip) on the GPU: every tensor of a rotated batch must equal FaceStore.host_batch(indices,
angles) -- the stated fixed-point algorithm, which tests/test_face_aug_cpu.py holds against its per-pixel formulas -- bit for bit:
the image half is integer arithmetic up to an exact float, the landmark half a float32 chain with nothing contracted, so there is
nothing to round differently and no tolerance.  Destinations are handed in prefilled (NaN, or a sentinel for the integer ones) with
guard cells on both sides that must come back untouched.

The stores are the smallest at which each mechanism can go wrong:
  s16        16 x 16, L = 9     every byte value, the hand-picked landmarks (negative, beyond 127, 1e6)
  23 x 37    L = 5              ragged rows (3 * 37 bytes), W != H, one row group shorter than 1024 pixels
  40 x 72    L = 2              three row groups of 14, 14 and 12 rows: the last one short
  128 x 128  L = 1027           the real geometry; crosses the 1024-landmark chunk
  8 x 2048   L = 3              a row group is ONE row here (W >= 1024).  Under any angle but 0 that row's taps span all 8 source
                                rows (2048 sin 1 deg = 36): a window of 64 KiB, beyond the 32 KiB of LDS, so the global-tap route; at
                                angle 0 the window is two rows, 16 KiB, staged in LDS.  The batches of all ten angles take both.
"""
import numpy as np
import pytest
import torch

import face_data_cases as fc
from ffwm_amd import data as fd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENTINEL = {torch.float32: float("nan"), torch.int64: -7777, torch.int32: -7}
ANGLES = list(range(-5, 5))
KEYS = fd.TRAIN_KEYS + ("invalid",)
_STORES = {}


def _stores(name):
    """(host store, device store, the rotation tables of [-5, 5) on the device, cache of host batches), built once per name."""
    if name not in _STORES:
        if name == "s16":
            c = fc.case("s16")
        else:
            H, W, L = {"23x37": (23, 37, 5), "40x72": (40, 72, 2), "128": (128, 128, 1027), "8x2048": (8, 2048, 3)}[name]
            c = fc.synthetic(3, H, W, L, seed=H * 1000 + W + L)
        host = fd.FaceStore.from_arrays(c["images"], c["masks"], c["names"], c["lm_dicts"], load_size=c["load_size"], rotation=True)
        dev = host.to(DEV)
        _STORES[name] = (host, dev, dev.rotation(-5, 5), {})
    return _STORES[name]


def _want(name, indices, angles):
    host, _, _, cache = _stores(name)
    key = (tuple(indices), tuple(angles))
    if key not in cache:
        w = host.host_batch(indices, angles)
        del w["input_path"]
        cache[key] = w
    return cache[key]


def _every_angle_and_flip(name, B):
    """B = 20: all ten angles on unflipped items, then on flipped ones; B = 1: a flipped item at -5 degrees."""
    host = _stores(name)[0]
    P = host.n_pairs
    if B == 1:
        return [P + 1], [-5]
    return [(j % P) + (j // 10) * P for j in range(20)], [ANGLES[j % 10] for j in range(20)]


def _guarded(B, store, keys=KEYS):
    _, H, W, _ = store.t["images"].shape
    L = store.t["lm"].shape[1]
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


def _i32(values):
    return torch.tensor(values, dtype=torch.int64).to(torch.int32).to(DEV)


@pytest.mark.parametrize("B", [20, 1])
@pytest.mark.parametrize("name", ["s16", "23x37", "40x72", "128", "8x2048"])
def test_rotated_batch_equals_host_batch(name, B):
    _, dev, rot, _ = _stores(name)
    indices, angles = _every_angle_and_flip(name, B)
    flats, out = _guarded(B, dev)
    res = dev.batch_rotated(_i32(indices), rot.slots(angles).to(DEV), rot, out=out)
    want = _want(name, indices, angles)
    assert set(res) == set(want) | {"invalid"} and len(want) == 7
    for k, w in want.items():
        assert res[k] is out[k] and res[k].dtype == w.dtype and res[k].shape == w.shape and torch.equal(res[k].cpu(), w), k
    assert res["invalid"].tolist() == [0] * B
    _guards_untouched(flats, out)
    if B == 20:
        plain = dev.batch(_i32(indices))
        assert not torch.equal(res["img_S"], plain["img_S"]) and torch.equal(res["img_F"], plain["img_F"])          # it did rotate
        # host angles on a device store take the same launch
        again = dev.batch(_i32(indices), angle=angles)
        assert all(torch.equal(again[k], res[k]) for k in KEYS)


def test_every_byte_value_passes_through_at_angle_zero():
    host, dev, rot, _ = _stores("s16")
    res = dev.batch_rotated(_i32([0]), rot.slots([0]).to(DEV), rot)
    assert res["img_S"][0].unique().numel() == 256
    assert torch.equal(res["img_S"].cpu(), host.host_batch([0])["img_S"])


@pytest.mark.parametrize("name", ["23x37", "8x2048"])
def test_out_of_range_index_and_slot_give_zeros_and_a_flag(name):
    _, dev, rot, _ = _stores(name)
    indices = [2, 12, 9, 4, -1, 7]          # 2 P = 12
    slots = [9, 3, 10, 0, 2, -1]            # A = 10
    good = [0, 3]
    flats, out = _guarded(len(indices), dev)
    res = dev.batch_rotated(_i32(indices), _i32(slots), rot, out=out)
    assert res["invalid"].tolist() == [0, 1, 1, 0, 1, 1]
    want = _want(name, [indices[j] for j in good], [slots[j] - 5 for j in good])
    for k in fd.TRAIN_KEYS:
        got = res[k].cpu()
        assert torch.equal(got[good], want[k]), k                                       # the neighbours are served
        assert bool((got[[1, 2, 4, 5]] == 0).all()), k                                  # (NaN prefill: a cell left unwritten is not 0)
    _guards_untouched(flats, out)


def test_out_is_written_in_place_and_a_short_batch_leaves_the_rest():
    name = "23x37"
    _, dev, rot, _ = _stores(name)
    flats, full = _guarded(5, dev)
    ptrs = {k: v.data_ptr() for k, v in full.items()}
    indices, angles = [7, 0, 11], [4, -5, 1]
    res = dev.batch_rotated(_i32(indices), rot.slots(angles).to(DEV), rot, out={k: v[:3] for k, v in full.items()})
    want = _want(name, indices, angles)
    for k in KEYS:
        assert res[k].data_ptr() == ptrs[k] and res[k].shape[0] == 3, k
        tail = full[k][3:]
        assert bool(torch.isnan(tail).all()) if tail.dtype == torch.float32 else bool((tail == SENTINEL[tail.dtype]).all()), k
    assert all(torch.equal(full[k][:3].cpu(), want[k]) for k in fd.TRAIN_KEYS) and full["invalid"][:3].tolist() == [0, 0, 0]
    _guards_untouched(flats, full)


def test_a_captured_launch_follows_the_index_and_slot_tensors():
    from ffwm_amd import graphs
    name = "s16"
    _, dev, rot, _ = _stores(name)
    first, second = ([0, 7, 3, 9], [4, -5, 0, 2]), ([8, 1, 1, 4], [-3, 3, -1, -5])
    index, slot = _i32(first[0]), rot.slots(first[1]).to(DEV)
    _, out = _guarded(4, dev)
    graphs.warm_up(lambda: dev.batch_rotated(index, slot, rot, out=out), 2, sync=True)
    g, _ = graphs.capture(lambda: dev.batch_rotated(index, slot, rot, out=out))
    g.replay()
    for k, w in _want(name, *first).items():
        assert torch.equal(out[k].cpu(), w), k
    index.copy_(_i32(second[0]))
    slot.copy_(rot.slots(second[1]).to(DEV))
    g.replay()
    for k, w in _want(name, *second).items():
        assert torch.equal(out[k].cpu(), w), k


def test_loader_epochs_equal_the_cpu_loader():
    host, dev, _, _ = _stores("23x37")
    on_gpu, on_cpu = fd.FaceLoader(dev, 4, rotation=True, seed=3), fd.FaceLoader(host, 4, rotation=True, seed=3)
    plain = fd.FaceLoader(dev, 4, seed=3)
    for epoch in (0, 1):
        got = [(b, {k: v.cpu() for k, v in b.items()}, b.invalid.cpu()) for b in on_gpu]          # (read before the buffers come round)
        want = list(on_cpu)
        paths = [b.input_path for b in plain]
        assert len(got) == len(want) == 3 and [b.batch_weight for b, _, _ in got] == [w.batch_weight for w in want] == [4, 4, 4]
        for (b, tensors, invalid), w, p in zip(got, want, paths):
            assert b.input_path == w.input_path == p and set(tensors) == set(w) == set(fd.TRAIN_KEYS)
            assert all(torch.equal(tensors[k], w[k]) for k in w) and invalid.tolist() == [0] * 4
        assert torch.equal(on_gpu.permutation(epoch), plain.permutation(epoch))
    assert len(set(torch.cat([on_gpu.draws(e)[1] for e in (0, 1)]).tolist())) > 1          # angles were drawn


@pytest.mark.parametrize("which", ["FlowNetTrainer", "FFWMTrainer"])
def test_a_trainer_takes_a_rotated_batch(which):
    """One eager step at ngf = 16, the smallest width the GPU trainer tests step at."""
    from ffwm_amd import trainer
    torch.backends.cudnn.benchmark = False
    if "trainer" not in _STORES:
        c = fc.synthetic(2, 128, 128, 1024, seed=3)
        _STORES["trainer"] = fd.FaceStore.from_arrays(c["images"], c["masks"], c["names"], c["lm_dicts"], rotation=True).to(DEV)
    batch = _STORES["trainer"].batch(_i32([1, 6]), angle=[4, -5])
    assert batch.pop("invalid").tolist() == [0, 0] and set(batch["mask_S"].unique().tolist()) <= {0.0, 1.0}
    t = getattr(trainer, which)(DEV, seed=0, ngf=16)
    t.step(batch)
    torch.cuda.synchronize()
    v = t.loss_values()
    assert v and all(torch.isfinite(torch.tensor(x)) for x in v.values()), v

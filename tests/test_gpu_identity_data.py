"""csrc/identity_batch.hip on the GPU against IdentityStore.host_batch -- the float64 restatement of PIL's rotation and the reference's
own torch calls, which tests/test_identity_data_cpu.py holds against PIL and against the recorded fixture.

Without crop every float must EQUAL the host's: the kernel's bytes are PIL's bytes and byte / 255, ((r + g) + b) / 3 are single
correctly rounded float32 operations.  With crop the plane is still exact and the bilinear resize is held against its float64
evaluation E: values lie in [0, 1], a result is four products and three sums of float32 with two float32 weights per axis, about
6 roundings of at most 2^-24 each, so |kernel - E| <= 2^-21 -- and ATen's own float32 result must stay inside that bound too.
Destinations are handed in prefilled with NaN (a sentinel for the integer ones) between guard cells that must come back untouched."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import identity_data_cases as ic
from ffwm_amd import data as fd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
N, B = 7, 5
CROP_BOUND = 2.0 ** -21
SENTINEL = {torch.float32: float("nan"), torch.int64: -7777, torch.int32: -7}
INDICES = [3, 0, 6, 3, 5]
FLIPS = [0, 1, 1, 0, 1]
_STORES = {}


def _stores(H, W):
    """(host store, device store, cache) of N images, built once per shape."""
    if (H, W) not in _STORES:
        names, images = ic.synthetic(N, H, W, seed=H * 1000 + W)
        host = fd.IdentityStore.from_arrays(images, names)
        _STORES[(H, W)] = (host, host.to(DEV), {})
    return _STORES[(H, W)]


def _matrices(H, W):
    """The angles 0, 5, -5, 1e-9 and a drawn one, as Image.rotate's matrices."""
    angles = [0.0, 5.0, -5.0, 1e-9, float(np.random.RandomState(H + W).uniform(-5, 5))]
    return [fd.rotation_matrix(a, W, H) for a in angles]


def _want(H, W, augment, crop):
    """The host's batch of INDICES, computed once per case and left unchanged."""
    host, _, cache = _stores(H, W)
    if (augment, crop) not in cache:
        cache[(augment, crop)] = host.host_batch(INDICES, flips=FLIPS if augment else None, crop=crop,
                                                 matrices=_matrices(H, W) if augment else None)
    return cache[(augment, crop)]


def _dev(values, dtype):
    return torch.tensor(values, dtype=dtype).to(DEV)


def _inputs(H, W, augment):
    index = _dev(INDICES, torch.int32)
    if not augment:
        return index, None, None
    return index, _dev(_matrices(H, W), torch.float64), _dev(FLIPS, torch.uint8)


def _guarded(b, side):
    shapes = {"img": ((b, 1) + side, torch.float32), "target": ((b,), torch.int64), "invalid": ((b,), torch.int32)}
    flats, out = {}, {}
    for k, (shape, dt) in shapes.items():
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


@pytest.mark.parametrize("augment", [True, False])
@pytest.mark.parametrize("hw", [(128, 128), (37, 53), (5, 4), (1, 1), (2, 9)])
def test_batch_equals_host_batch_exactly(hw, augment):
    H, W = hw
    _, dev, _ = _stores(H, W)
    flats, out = _guarded(B, (H, W))
    res = dev.batch(*_inputs(H, W, augment), crop=False, out=out)
    want = _want(H, W, augment, False)
    assert set(res) == {"img", "target", "invalid"} and all(res[k] is out[k] for k in out)
    assert res["img"].dtype == torch.float32 and torch.equal(res["img"].cpu(), want["img"])          # no pixel may differ
    assert torch.equal(res["target"].cpu(), want["target"]) and res["invalid"].tolist() == [0] * B
    _guards_untouched(flats, out)


def test_the_rotation_moves_pixels():
    """The exactness test is not a comparison of two identities: 5 degrees at 128 x 128 changes most of the plane."""
    plain, turned = _want(128, 128, False, False)["img"], _want(128, 128, True, False)["img"]
    assert torch.equal(plain[0], turned[0]) and float((plain[1] != turned[1]).float().mean()) > 0.9          # angle 0; angle 5 + flip


@pytest.mark.parametrize("augment", [True, False])
@pytest.mark.parametrize("hw", [(40, 47), (128, 128)])
def test_crop_within_the_float64_bound(hw, augment):
    H, W = hw
    _, dev, _ = _stores(H, W)
    flats, out = _guarded(B, (128, 128))
    res = dev.batch(*_inputs(H, W, augment), crop=True, out=out)
    plane = _want(H, W, augment, False)["img"]                                        # float32, exact by the test above
    E = F.interpolate(plane.double()[:, :, 28:-2, 15:-15], (128, 128), mode="bilinear")
    got = res["img"].cpu()
    assert tuple(got.shape) == (B, 1, 128, 128) and not bool(torch.isnan(got).any())
    err, aten = (got.double() - E).abs().max().item(), (_want(H, W, augment, True)["img"].double() - E).abs().max().item()
    print("crop %dx%d augment %d: |kernel - E| = %.3g 2^-24, |ATen - E| = %.3g 2^-24" % (H, W, augment, err * 2 ** 24, aten * 2 ** 24))
    assert err <= CROP_BOUND and aten <= CROP_BOUND
    assert float(E.max()) > 0.5          # (not a plane of zeros)
    assert torch.equal(res["target"].cpu(), _want(H, W, augment, True)["target"]) and res["invalid"].tolist() == [0] * B
    _guards_untouched(flats, out)


@pytest.mark.parametrize("hw,crop", [((37, 53), False), ((40, 47), True)])
def test_invalid_samples_give_zeros_and_a_flag(hw, crop):
    H, W = hw
    host, dev, _ = _stores(H, W)
    idx = [-1, 2, N, 4, 1, 5, 2 ** 31 - 1, -2 ** 31]
    ms = [fd.rotation_matrix(a, W, H) for a in (3.0, -4.0, 1.0, 2.0, -1.5, 5.0, 0.5, -0.5)]
    ms[3][4] = float("nan")
    ms[4][5] = float("inf")
    flips = [1, 1, 0, 0, 1, 0, 1, 0]
    flats, out = _guarded(len(idx), (128, 128) if crop else (H, W))
    res = dev.batch(_dev(idx, torch.int32), _dev(ms, torch.float64), _dev(flips, torch.uint8), crop=crop, out=out)
    assert res["invalid"].tolist() == [1, 0, 1, 1, 1, 0, 1, 1]
    img, target = res["img"].cpu(), res["target"].cpu()
    bad, good = [0, 2, 3, 4, 6, 7], [1, 5]
    assert bool((img[bad] == 0).all()) and target[bad].tolist() == [0] * 6          # (NaN prefill: a cell left unwritten is not 0)
    want = host.host_batch([2, 5], flips=[1, 0], crop=False, matrices=[ms[1], ms[5]])
    assert target[good].tolist() == want["target"].tolist() == [1, 2]
    if crop:
        E = F.interpolate(want["img"].double()[:, :, 28:-2, 15:-15], (128, 128), mode="bilinear")
        assert (img[good].double() - E).abs().max().item() <= CROP_BOUND
    else:
        assert torch.equal(img[good], want["img"])          # the neighbours are served, bit for bit
    _guards_untouched(flats, out)


def test_any_finite_matrix_is_safe():
    """Matrices far outside a rotation: everything maps outside the image, or onto one source pixel; nothing is read out of bounds."""
    H, W = 5, 4
    host, dev, _ = _stores(H, W)
    ms = [[1e300, 0, 0, 0, 1e300, 0], [0, 0, -1e9, 0, 0, 2.0], [1e308, 1e308, 1e308, -1e308, -1e308, 1e308], [0, 0, 2.5, 0, 0, 1.5],
          [-1.0, 0, 4.0, 0, -1.0, 5.0]]
    flats, out = _guarded(5, (H, W))
    res = dev.batch(_dev([0, 1, 2, 3, 4], torch.int32), _dev(ms, torch.float64), _dev([0] * 5, torch.uint8), crop=False, out=out)
    want = host.host_batch([0, 1, 2, 3, 4], matrices=ms)
    assert torch.equal(res["img"].cpu(), want["img"]) and res["invalid"].tolist() == [0] * 5
    assert not bool(want["img"][:3].any()) and want["img"][3].unique().numel() == 1 and bool(want["img"][4].any())
    _guards_untouched(flats, out)


def test_a_short_batch_leaves_the_remaining_rows():
    H, W = 37, 53
    _, dev, _ = _stores(H, W)
    index, matrix, flip = _inputs(H, W, True)
    for crop, side in ((False, (H, W)), (True, (128, 128))):
        flats, out = _guarded(B, side)
        res = dev.batch(index[:3], matrix[:3], flip[:3], crop=crop, out={k: v[:3] for k, v in out.items()})
        assert not bool(torch.isnan(res["img"]).any()) and res["img"].data_ptr() == out["img"].data_ptr()
        assert bool(torch.isnan(out["img"][3:]).all()) and out["target"][3:].tolist() == [-7777] * 2 and out["invalid"][3:].tolist() == [-7] * 2
        assert res["target"].tolist() == _want(H, W, True, False)["target"][:3].tolist() and res["invalid"].tolist() == [0] * 3
        if not crop:
            assert torch.equal(res["img"].cpu(), _want(H, W, True, False)["img"][:3])
        _guards_untouched(flats, out)


def test_two_calls_are_bit_identical():
    for (H, W), crop in (((128, 128), False), ((128, 128), True), ((40, 47), True)):
        _, dev, _ = _stores(H, W)
        args = _inputs(H, W, True)
        a, b = dev.batch(*args, crop=crop), dev.batch(*args, crop=crop)
        assert a["img"].data_ptr() != b["img"].data_ptr() and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("crop", [False, True])
def test_a_captured_launch_follows_its_device_inputs(crop):
    from ffwm_amd import graphs
    H, W = 40, 47
    host, dev, _ = _stores(H, W)
    index, matrix, flip = _inputs(H, W, True)
    _, out = _guarded(B, (128, 128) if crop else (H, W))
    graphs.warm_up(lambda: dev.batch(index, matrix, flip, crop=crop, out=out), 2, sync=True)
    g, _ = graphs.capture(lambda: dev.batch(index, matrix, flip, crop=crop, out=out))

    def check(indices, ms, flips):
        want = host.host_batch(indices, flips=flips, crop=False, matrices=ms)
        got = out["img"].cpu()
        if crop:
            E = F.interpolate(want["img"].double()[:, :, 28:-2, 15:-15], (128, 128), mode="bilinear")
            assert (got.double() - E).abs().max().item() <= CROP_BOUND
        else:
            assert torch.equal(got, want["img"])
        assert torch.equal(out["target"].cpu(), want["target"]) and out["invalid"].tolist() == [0] * B

    g.replay()
    check(INDICES, _matrices(H, W), FLIPS)
    second, ms2, flips2 = [1, 1, 4, 2, 0], [fd.rotation_matrix(a, W, H) for a in (-3.25, 4.5, 0.0, 2.0, -5.0)], [1, 0, 0, 1, 1]
    index.copy_(_dev(second, torch.int32))
    matrix.copy_(_dev(ms2, torch.float64))
    flip.copy_(_dev(flips2, torch.uint8))
    g.replay()
    check(second, ms2, flips2)


def test_loader_epoch_and_its_buffers():
    H, W = 40, 47
    host, dev, _ = _stores(H, W)
    loader = fd.IdentityLoader(dev, 3, crop=False, seed=3)
    batches = []
    for b in loader:
        batches.append((b, {k: v.cpu() for k, v in b.items()}))          # (read before the batch after next overwrites it)
    perm, angles, flips = loader.draws(0)
    assert [b.batch_weight for b, _ in batches] == [3, 3, 1]
    for s, (b, got) in enumerate(batches):
        lo, hi = 3 * s, min(N, 3 * s + 3)
        want = host.host_batch(perm[lo:hi].tolist(), angles[lo:hi].tolist(), flips[lo:hi].tolist())
        assert b.input_path == want["input_path"] and set(got) == {"img", "target"}
        assert torch.equal(got["img"], want["img"]) and torch.equal(got["target"], want["target"])
    ptrs = [b["img"].data_ptr() for b, _ in batches]
    assert ptrs[0] != ptrs[1] and ptrs[2] == ptrs[0]          # two buffer sets, used alternately
    assert torch.cat([b.invalid for b, _ in batches]).tolist() == [0] * N
    # `out`: every full batch lands in the caller's tensors; a validation store is sequential and plain
    static = {"img": torch.empty(3, 1, 128, 128, device=DEV), "target": torch.empty(3, dtype=torch.int64, device=DEV)}
    val = fd.IdentityStore.from_arrays(host.t["images"], host.names, isval=True).to(DEV)
    for s, b in enumerate(fd.IdentityLoader(val, 3, crop=True, drop_last=True, out=static)):
        assert b["img"] is static["img"] and b["target"] is static["target"] and b.input_path == host.names[3 * s:3 * s + 3]
        E = F.interpolate(host.host_batch([3 * s, 3 * s + 1, 3 * s + 2])["img"].double()[:, :, 28:-2, 15:-15], (128, 128), mode="bilinear")
        assert (static["img"].cpu().double() - E).abs().max().item() <= CROP_BOUND
    assert set(static) == {"img", "target"}          # the caller's dict is left as it was


def test_from_face_store_shares_the_device_images():
    import face_data_cases as fc
    c = fc.synthetic(2, 16, 16, 1, seed=5)
    face = fd.FaceStore.from_arrays(c["images"], c["masks"], c["names"], c["lm_dicts"]).to(DEV)
    store = fd.IdentityStore.from_face_store(face)
    assert store.t["images"].data_ptr() == face.t["images"].data_ptr() and store.device.type == "cuda"
    res = store.batch(_dev([3, 0], torch.int32))
    assert torch.equal(res["img"].cpu(), store.host.host_batch([3, 0])["img"]) and res["target"].tolist() == [1, 0]


def test_a_trainer_step_on_the_loaders_batch():
    """LightCNNTrainer.step takes the loader's batch as it is: the same loss bits as a step on the host's batch copied to the device."""
    from ffwm_amd import trainer
    host, dev, _ = _stores(128, 128)
    mask = ((torch.rand(2, 256, generator=torch.Generator().manual_seed(1)) > 0.3).float() / 0.7).to(DEV)
    loader = fd.IdentityLoader(dev, 2, seed=4)
    batch = next(iter(loader))
    perm, angles, flips = loader.draws(0)
    want = host.host_batch(perm[:2].tolist(), angles[:2].tolist(), flips[:2].tolist())
    assert batch.input_path == want["input_path"] and torch.equal(batch["img"].cpu(), want["img"])
    losses = []
    for b in (batch, {"img": want["img"].to(DEV), "target": want["target"].to(DEV)}):
        tr = trainer.LightCNNTrainer(DEV, num_classes=16, seed=2)
        losses.append(tr.step(b, dropout_mask=mask)["loss"].cpu())
    assert torch.isfinite(losses[0]) and torch.equal(losses[0], losses[1])


def test_train_epoch_with_a_captured_step():
    """train_epoch over a loader that writes into the captured step's static inputs: the means it reads back once at the end are the
    batch-size-weighted means of the per-step values (collected here step by step), and a batch of another size is refused."""
    from ffwm_amd import trainer
    _, dev, _ = _stores(128, 128)
    mask = ((torch.rand(2, 256, generator=torch.Generator().manual_seed(1)) > 0.3).float() / 0.7).to(DEV)
    tr = trainer.LightCNNTrainer(DEV, num_classes=16, seed=2, capturable=True)
    tr.capture(next(iter(fd.IdentityLoader(dev, 2, drop_last=True))), dropout_mask=mask)
    static = tr._static.tensors
    seen = []

    def batches(loader, in_place=True):
        for b in loader:
            assert not in_place or (b["img"] is static["img"] and b["target"] is static["target"])          # assembled where the graph reads
            b["dropout_mask"] = mask
            yield b
            seen.append([float(tr.losses[k]) for k in ("loss", "prec1", "prec5")])

    out = {"img": static["img"], "target": static["target"]}
    got = tr.train_epoch(batches(fd.IdentityLoader(dev, 2, drop_last=True, seed=6, out=out)), 1)
    assert len(seen) == 3 and all(np.isfinite(v) for row in seen for v in row)
    sums = [0.0, 0.0, 0.0]
    for row in seen:
        for i, v in enumerate(row):
            sums[i] += v * 2
    assert list(got) == [s / 6 for s in sums] and seen[0] != seen[2]
    with pytest.raises(ValueError, match="drop_last"):
        tr.train_epoch(batches(fd.IdentityLoader(dev, 2, seed=6), in_place=False), 2)          # N = 7: the last batch has one sample
    tr.release_graphs()

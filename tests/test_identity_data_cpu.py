"""ffwm_amd.data's LightCNN fine-tuning pipeline on the CPU: the float64 restatement of PIL's bicubic rotation against PIL itself and
against what PIL recorded in tests/golden/pil_bicubic_rotate.npz (byte for byte), the item arithmetic against the literal calls of
lightcnn/dataset.py:57-67, IdentityLoader's epochs, the storage forms, the argument checks of ffwm_identity_batch (which return before
any launch) and LightCNNTrainer.train_epoch against the hand-rolled loop."""
import ctypes
import os

import numpy as np
import pytest
import torch

import face_data_cases as fc
import identity_data_cases as ic
from ffwm_amd import data as fd

HERE = os.path.dirname(os.path.abspath(__file__))


def _restated(img, angle, flip):
    H, W, _ = img.shape
    out = fd.rotate_bicubic(img, fd.rotation_matrix(angle, W, H))
    return out[:, ::-1] if flip else out


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(HERE, "golden", "pil_bicubic_rotate.npz")) as z:
        return {k: z[k] for k in z.files}


def _store(N=7, H=40, W=47, isval=False, seed=1):
    names, images = ic.synthetic(N, H, W, seed)
    return fd.IdentityStore.from_arrays(images, names, isval=isval)


# ---------------------------------------------------------------------------------------------------------------- the rotation
def test_the_restatement_equals_pil():
    Image = pytest.importorskip("PIL.Image")
    cases = ic.cases()
    assert len(cases) == 140
    for key, img, angle, flip in cases:
        want = Image.fromarray(img).rotate(angle, resample=Image.BICUBIC, expand=False)
        if flip:
            want = want.transpose(Image.FLIP_LEFT_RIGHT)
        assert np.array_equal(_restated(img, angle, flip), np.asarray(want)), key


def test_the_restatement_equals_the_recorded_fixture(golden):
    cases = {c[0]: c for c in ic.golden_cases()}
    keys = [str(k) for k in golden["keys"]]
    assert keys == list(cases) and len(keys) == 114 and sum(k.startswith("128x128") for k in keys) == 2
    rotated = 0
    for key, angle, flip in zip(keys, golden["angles"].tolist(), golden["flips"].tolist()):
        _, img, a, f = cases[key]
        assert a == angle and f == flip and np.array_equal(img, golden["in/" + key]), key          # the generator's inputs are the file's
        want = golden["out/" + key]
        assert np.array_equal(_restated(img, angle, flip), want), key
        rotated += int(not np.array_equal(want, img[:, ::-1] if flip else img))
    assert rotated >= 60          # (the fixture is not a list of identities: 1 x 1 images and the angles 0 and 1e-9 are)


def test_the_cubic_is_the_sharp_one_and_the_byte_is_truncated(golden):
    """What the restatement must not be confused with: rounding to nearest instead of truncating changes the recorded bytes."""
    key = "37x53_random_1"
    img, want = golden["in/" + key], golden["out/" + key]
    m = fd.rotation_matrix(5.0, 53, 37)
    assert np.array_equal(fd.rotate_bicubic(img, m), want)
    assert 0.99 < m[0] == m[4] < 1.0 and m[1] == -m[3] and m[2] != 0.0 and all(v == round(v, 15) for v in (m[0], m[1]))
    assert want.min() == 0 and want.max() == 255          # the clip acts (the a = -1 cubic overshoots on random bytes)


def test_any_finite_matrix_is_served():
    img = ic.image("random", 5, 4, np.random.RandomState(0))
    for m in ([1e300, 0, 0, 0, 1e300, 0], [0, 0, -1e9, 0, 0, 2.0], [1e308, 1e308, 1e308, -1e308, -1e308, 1e308]):
        assert not fd.rotate_bicubic(img, m).any()          # everything maps outside
    assert np.array_equal(fd.rotate_bicubic(img, [1, 0, 0, 0, 1, 0]), img)
    assert np.array_equal(fd.rotate_bicubic(img, [0, 0, 2.5, 0, 0, 1.5]), np.broadcast_to(img[1, 2], img.shape))          # one source pixel


# ---------------------------------------------------------------------------------------------------------------- the item
@pytest.mark.parametrize("crop", [False, True])
def test_items_equal_the_literal_calls_of_the_reference(golden, crop):
    key = "128x128_random_2"
    names, images = ic.synthetic(3, 128, 128, 4)
    images[1] = golden["in/" + key]
    store = fd.IdentityStore.from_arrays(images, names)

    def postprocess(img):          # dataset.py:62-67
        img = torch.mean(img, dim=(0, ), keepdim=True)
        if crop:
            img = img[:, 28:-2, 15:-15]
            img = torch.nn.functional.interpolate(img.unsqueeze(0), (128, 128), mode='bilinear')
            img = img[0]
        return img

    # a test item: get_test_item + postprocess(train=False)
    img = torch.from_numpy(images[2].copy().astype('float32').transpose((2, 0, 1)).astype('float32'))
    want = postprocess(img.float().div(255))
    got = store.host_item(2, crop=crop)
    assert got["img"].dtype == torch.float32 and tuple(got["img"].shape) == (1, 128, 128) and torch.equal(got["img"], want)
    assert got["input_path"] == names[2] and int(got["target"]) == 1
    # a training item: ToTensor of PIL's recorded bytes (HWC bytes -> CHW, float, div(255)), then postprocess
    angle, flip = float(golden["angles"][list(golden["keys"]).index(key)]), bool(golden["flips"][list(golden["keys"]).index(key)])
    pil = torch.from_numpy(golden["out/" + key]).permute((2, 0, 1)).contiguous().to(dtype=torch.float32).div(255)
    got = store.host_item(1, angle=angle, flip=flip, crop=crop)["img"]
    assert torch.equal(got, postprocess(pil))
    if not crop:
        # the channel mean is ((r + g) + b) / 3 in float32: the arithmetic of the kernels
        b = golden["out/" + key].astype(np.float32) / np.float32(255)
        assert np.array_equal(got[0].numpy(), ((b[..., 0] + b[..., 1]) + b[..., 2]) / np.float32(3))


def test_host_batch_collates_items():
    store = _store()
    b = store.host_batch([3, 0, 3], angles=[5.0, -2.5, 0.0], flips=[True, False, False], crop=True)
    assert tuple(b["img"].shape) == (3, 1, 128, 128) and b["target"].dtype == torch.int64 and b["target"].tolist() == [1, 0, 1]
    assert b["input_path"] == [store.names[3], store.names[0], store.names[3]]
    assert torch.equal(b["img"][1], store.host_item(0, angle=-2.5, crop=True)["img"])
    assert torch.equal(b["img"][2], store.host_item(3, crop=True)["img"])          # a rotation by 0 is the identity
    assert not torch.equal(b["img"][0], b["img"][2])
    with pytest.raises(IndexError):
        store.host_item(7)
    one = _store(N=2, H=1, W=1)          # a single pixel: rotated and flipped it is itself
    assert torch.equal(one.host_item(1, angle=5.0, flip=True)["img"], one.host_item(1)["img"])
    res = store.batch([3, 0], [fd.rotation_matrix(5.0, 47, 40), fd.rotation_matrix(-2.5, 47, 40)], [1, 0], crop=True)
    assert set(res) == {"img", "target", "invalid"} and torch.equal(res["img"], b["img"][:2]) and res["invalid"].tolist() == [0, 0]


# ---------------------------------------------------------------------------------------------------------------- the loader
def test_loader_epochs():
    from ffwm_amd.trainer import LightCNNTrainer
    store = _store(N=7)
    loader = fd.IdentityLoader(store, 3, seed=5, degrees=5.0)
    assert len(loader) == 3 and len(fd.IdentityLoader(store, 3, drop_last=True)) == 2 and loader.shuffle and loader.augment
    p0, a0, f0 = loader.draws(0)
    p0b, a0b, f0b = fd.IdentityLoader(store, 2, seed=5).draws(0)
    assert torch.equal(p0, p0b) and torch.equal(a0, a0b) and torch.equal(f0, f0b)          # same seed and epoch
    p1, a1, f1 = loader.draws(1)
    assert not torch.equal(p0, p1) and not torch.equal(a0, a1)
    assert torch.equal(p1, fd.IdentityLoader(store, 3, seed=6).draws(0)[0])                # seed + epoch
    assert p0.dtype == torch.int32 and sorted(p0.tolist()) == list(range(7))
    assert a0.dtype == torch.float64 and float(a0.abs().max()) <= 5.0 and a0.unique().numel() == 7 and f0.dtype == torch.uint8
    wide = fd.IdentityLoader(store, 3, seed=5, degrees=30.0).draws(0)[1]
    assert float(wide.abs().max()) <= 30.0 and float(wide.abs().max()) > 5.0
    # the draws follow the order permutation, angles, flips under one generator
    g = torch.Generator().manual_seed(5)
    assert torch.equal(torch.randperm(7, generator=g).to(torch.int32), p0)
    assert torch.equal((torch.rand(7, dtype=torch.float64, generator=g) * 2.0 - 1.0) * 5.0, a0)
    assert torch.equal((torch.rand(7, generator=g) < 0.5).to(torch.uint8), f0)
    batches = list(loader)
    assert [b.batch_weight for b in batches] == [3, 3, 1] and loader.epoch == 1
    for s, b in enumerate(batches):
        lo, hi = 3 * s, min(7, 3 * s + 3)
        want = store.host_batch(p0[lo:hi].tolist(), a0[lo:hi].tolist(), f0[lo:hi].tolist())
        assert set(b) == {"img", "target"} and torch.equal(b["img"], want["img"]) and torch.equal(b["target"], want["target"])
        assert b.input_path == want["input_path"] and torch.equal(b["target"], LightCNNTrainer.targets_from_names(b.input_path))
        assert b.invalid.tolist() == [0] * (hi - lo)
    assert torch.equal(loader.matrices(a0)[2], torch.tensor(fd.rotation_matrix(float(a0[2]), 47, 40), dtype=torch.float64))
    second = list(loader)          # the next epoch
    assert torch.equal(torch.cat([b["target"] for b in second]), store.t["targets"][p1.long()])


def test_a_validation_loader_is_sequential_and_plain():
    store = _store(N=5, isval=True)
    loader = fd.IdentityLoader(store, 2, crop=True)
    assert not loader.shuffle and not loader.augment and loader.draws(3)[1] is None
    batches = list(loader)
    assert [b.input_path for b in batches] == [store.names[0:2], store.names[2:4], store.names[4:5]]
    assert torch.equal(batches[1]["img"], store.host_batch([2, 3], crop=True)["img"]) and tuple(batches[2]["img"].shape) == (1, 1, 128, 128)


# ---------------------------------------------------------------------------------------------------------------- storage
def test_from_face_store_shares_the_images():
    c = fc.case("s16")
    face = fd.FaceStore.from_arrays(c["images"], c["masks"], c["names"], c["lm_dicts"], load_size=16)
    store = fd.IdentityStore.from_face_store(face)
    assert store.t["images"].data_ptr() == face.t["images"].data_ptr() and store.names == face.names and not store.isval
    assert store.t["targets"].tolist() == [0, 0, 1, 1, 0] and store.gallery_names is None and len(store) == 5
    val = fd.IdentityStore.from_face_store(fd.FaceStore.from_arrays(c["images"], None, c["names"], isval=True, load_size=16))
    assert val.isval and val.gallery_names == ["001_01_01_051_06.png", "002_01_01_051_06.png"]


def test_gallery_as_face_store_has_it():
    c = fc.case("s16")
    face = fd.FaceStore.from_arrays(c["images"], None, c["names"], isval=True, load_size=16)
    store = fd.IdentityStore.from_arrays(c["images"], c["names"], isval=True)
    ids, planes = store.gallery()
    want_ids, want = face.host_gallery()
    assert ids == want_ids == ["001", "002"] and torch.equal(planes, want)
    listed = fd.IdentityStore.from_arrays(c["images"], c["names"], isval=True, gallery_list=[c["names"][4]])
    assert listed.gallery()[0] == ["001"] and torch.equal(listed.gallery()[1][0], store.host_item(4)["img"])
    with pytest.raises(ValueError):
        fd.IdentityStore.from_arrays(c["images"], c["names"]).gallery()
    with pytest.raises(KeyError):
        fd.IdentityStore.from_arrays(c["images"], c["names"], isval=True, gallery_list=["003_01_01_051_06.png"])
    with pytest.raises(ValueError, match="three-digit"):
        fd.IdentityStore.from_arrays(c["images"][:1], ["face.png"])


def test_npz_round_trip(tmp_path):
    for isval in (False, True):
        store = _store(N=4, H=5, W=4, isval=isval)
        path = str(tmp_path / ("set%d.npz" % isval))
        store.save(path)
        back = fd.IdentityStore.load(path)
        assert back.names == store.names and back.isval == isval and back.gallery_names == store.gallery_names
        assert torch.equal(back.t["images"], store.t["images"]) and torch.equal(back.t["targets"], store.t["targets"])
        assert back.t["targets"].dtype == torch.int64 and (back.gallery_names is None) == (not isval)


def test_directory_round_trip(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    names, images = ic.synthetic(4, 5, 4, 2)
    for split in ("train", "test"):
        os.makedirs(str(tmp_path / split / "images"))
        for n, im in zip(names, images):
            Image.fromarray(im).save(str(tmp_path / split / "images" / n))
    np.save(str(tmp_path / "test" / "gallery_list.npy"), np.array([names[2]]))
    train = fd.IdentityStore.from_directory(str(tmp_path), threads=2)
    assert train.names == sorted(names) and not train.isval and train.gallery_names is None
    assert np.array_equal(train.t["images"].numpy(), images[[names.index(n) for n in train.names]])
    test = fd.IdentityStore.from_directory(str(tmp_path), isval=True)
    assert test.isval and test.gallery_names == [names[2]]
    Image.fromarray(images[0][..., 0]).save(str(tmp_path / "train" / "images" / names[0]))
    with pytest.raises(ValueError, match="RGB"):
        fd.IdentityStore.from_directory(str(tmp_path))


def test_lazy_exports():
    import ffwm_amd
    assert ffwm_amd.IdentityStore is fd.IdentityStore and ffwm_amd.IdentityLoader is fd.IdentityLoader
    assert ffwm_amd.IdentityBatch is fd.IdentityBatch


# ---------------------------------------------------------------------------------------------------------------- the C entry point
def test_cpu_tensors_are_refused_by_the_op():
    from ffwm_amd import ops
    store = _store()
    with pytest.raises(NotImplementedError):
        ops.identity_batch(store.t["images"], store.t["targets"], torch.zeros(1, dtype=torch.int32))


def test_entry_point_refuses_bad_arguments_before_any_launch():
    from ffwm_amd import build, _lib
    build.build()
    lib = _lib.load()
    assert hasattr(lib, "ffwm_identity_batch") and "ffwm_identity_batch" in _lib.EXPORTS
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(images=p, targets=p, index=p, matrix=p, flip=p, img=p, target=p, invalid=p, N=4, H=40, W=47, B=2, out_side=128,
                augment=1, crop=1)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ffwm_identity_batch(*[a[k] for k in good], None)

    for k in ("images", "targets", "index", "matrix", "flip", "img", "target", "invalid"):
        assert call(**{k: None}) == -1 and b"NULL" in lib.ffwm_last_error(), k
    for k in ("images", "targets", "index", "img", "target", "invalid"):
        assert call(augment=0, matrix=None, flip=None, **{k: None}) == -1 and b"NULL" in lib.ffwm_last_error(), k
    for k in ("N", "H", "W", "B", "out_side"):
        for v in (0, -1):
            assert call(**{k: v}) == -1 and b"positive" in lib.ffwm_last_error(), (k, v)
    for k in ("augment", "crop"):
        for v in (2, -1):
            assert call(**{k: v}) == -1 and b"0 or 1" in lib.ffwm_last_error(), (k, v)
    for kw in (dict(H=30), dict(W=30), dict(H=1), dict(H=30, W=30)):
        assert call(**kw) == -1 and b"exceed 30" in lib.ffwm_last_error(), kw
    assert call(W=8193) == -3 and call(H=8193) == -3 and call(out_side=8193) == -3 and b"8192" in lib.ffwm_last_error()
    assert call(B=65536) == -3 and call(N=1 << 31) == -3
    assert call(H=8192, W=8192, out_side=8) == -3 and b"LDS" in lib.ffwm_last_error()          # a band would read 8162 rows


# ---------------------------------------------------------------------------------------------------------------- the epoch
def test_train_epoch_equals_the_hand_rolled_loop():
    from ffwm_amd import trainer
    names, images = ic.synthetic(4, 128, 128, 8)          # identities 1 and 2 -> classes 0 and 1
    store = fd.IdentityStore.from_arrays(images, names)
    a, b = (trainer.LightCNNTrainer("cpu", num_classes=7, lr=1e-2, seed=3) for _ in range(2))
    torch.manual_seed(9)          # (F.dropout's draws)
    got = a.train_epoch(fd.IdentityLoader(store, 3, crop=True, seed=2), 25)
    torch.manual_seed(9)
    rates = b.adjust_learning_rate(25)
    sums, count = [0.0, 0.0, 0.0], 0
    batches = list(fd.IdentityLoader(store, 3, crop=True, seed=2))
    assert [x.batch_weight for x in batches] == [3, 1]
    for batch in batches:
        out = b.step(batch)
        for i, k in enumerate(("loss", "prec1", "prec5")):          # AverageMeter.update(val.item(), n)
            sums[i] += out[k].item() * batch.batch_weight
        count += batch.batch_weight
    assert isinstance(got, tuple) and list(got) == [s / count for s in sums] and got[0] > 0
    assert rates[0] == pytest.approx(1e-2 * trainer.LightCNNTrainer.LR_SCALE) and [g["lr"] for g in a.optimizer.param_groups] == rates
    for p, q in zip(a.net.parameters(), b.net.parameters()):
        assert torch.equal(p, q)
    with pytest.raises(ValueError, match="no batch"):
        a.train_epoch([], 0)

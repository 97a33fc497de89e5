"""The rotation of --aug on the CPU (ffwm_amd.data: rotation_tables, warp_affine_linear, rotate_landmarks, FaceStore / FaceLoader with
rotation=): the stated fixed-point algorithm against a per-pixel restatement in Python integers, against exact float64 bilinear
sampling within a derived bound, and against the landmark formula; the draws of the loader; the storage forms; the argument checks of
ffwm_face_batch_aug (which return before any launch).  No OpenCV was at hand: the comparison with cv2's own output runs only where
tests/golden/cv2_warp_affine.npz exists (tests/golden/make_face_aug_golden.py writes it where cv2 is installed)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import face_data_cases as fc
from ffwm_amd import data as fd

HERE = os.path.dirname(os.path.abspath(__file__))
ANGLES = list(range(-5, 5))          # np.random.randint(-5, 5)


def _store(c, **kw):
    return fd.FaceStore.from_arrays(c["images"], c["masks"], c["names"], c["lm_dicts"], load_size=c["load_size"], **kw)


@pytest.fixture(scope="module")
def s16():
    return _store(fc.case("s16"), rotation=True)


def test_tables_at_angle_zero_are_the_identity():
    rs = np.random.RandomState(0)
    for H, W in ((16, 16), (40, 72), (8, 2048)):
        t = fd.rotation_tables(0, W, H)
        assert all(v.dtype == np.int64 for v in t[:4])
        assert np.array_equal(t.adelta, 1024 * np.arange(W)) and np.array_equal(t.bdelta, np.zeros(W, dtype=np.int64))
        assert np.array_equal(t.X0, np.full(H, 16)) and np.array_equal(t.Y0, 1024 * np.arange(H) + 16)
        for shape in ((H, W), (H, W, 3)):
            img = rs.randint(0, 256, shape).astype(np.uint8)
            assert np.array_equal(fd.warp_affine_linear(img, t), 1024 * img.astype(np.int64))


def _scalar_warp(img, t):
    """The per-pixel formulas in plain Python integers."""
    H, W = len(img), len(img[0])
    p = lambda y, x: img[y][x] if 0 <= y < H and 0 <= x < W else 0          # noqa: E731 (BORDER_CONSTANT 0)
    ad, bd, X0, Y0 = (v.tolist() for v in t[:4])
    out = [[0] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            X, Y = (X0[y] + ad[x]) >> 5, (Y0[y] + bd[x]) >> 5
            sx, sy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31
            out[y][x] = (p(sy, sx) * (32 - fx) * (32 - fy) + p(sy, sx + 1) * fx * (32 - fy) + p(sy + 1, sx) * (32 - fx) * fy
                         + p(sy + 1, sx + 1) * fx * fy)
    return out


def test_vectorised_warp_equals_the_scalar_formulas():
    c = fc.case("s16")
    assert all((32 - fx) * (32 - fy) + fx * (32 - fy) + (32 - fx) * fy + fx * fy == 1024 for fx in range(32) for fy in range(32))
    for ang in ANGLES:
        t = fd.rotation_tables(ang, 16, 16)
        for flip in (False, True):
            image = c["images"][0][:, ::-1] if flip else c["images"][0]
            mask = c["masks"][0][:, ::-1] if flip else c["masks"][0]
            got = fd.warp_affine_linear(image, t)
            assert got.dtype == np.int64 and got.shape == (16, 16, 3)
            for ch in range(3):
                assert got[:, :, ch].tolist() == _scalar_warp(image[:, :, ch].tolist(), t), (ang, flip, ch)
            assert fd.warp_affine_linear(mask, t).tolist() == _scalar_warp(mask.tolist(), t), (ang, flip)
            assert int(got.max()) <= 255 * 1024


def _exact_bilinear(img, M):
    """Zero-padded float64 bilinear sampling at the inverse-mapped point, and the largest horizontal / vertical neighbour difference
    (Dx, Dy) over the 4 x 4 cells around it."""
    H, W = img.shape
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    u, v = M[0] * xs + M[1] * ys + M[2], M[3] * xs + M[4] * ys + M[5]
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    a, b = u - x0, v - y0
    P = np.pad(img.astype(np.float64), 3)

    def g(yy, xx):
        return P[np.clip(yy + 3, 0, H + 5), np.clip(xx + 3, 0, W + 5)]
    val = g(y0, x0) * (1 - a) * (1 - b) + g(y0, x0 + 1) * a * (1 - b) + g(y0 + 1, x0) * (1 - a) * b + g(y0 + 1, x0 + 1) * a * b
    Dx, Dy = np.zeros_like(val), np.zeros_like(val)
    for j in range(-1, 3):
        for i in range(-1, 3):
            Dx = np.maximum(Dx, np.maximum(np.abs(g(y0 + j, x0 + i + 1) - g(y0 + j, x0 + i)), np.abs(g(y0 + j, x0 + i) - g(y0 + j, x0 + i - 1))))
            Dy = np.maximum(Dy, np.maximum(np.abs(g(y0 + j + 1, x0 + i) - g(y0 + j, x0 + i)), np.abs(g(y0 + j, x0 + i) - g(y0 + j - 1, x0 + i))))
    return val, Dx, Dy


@pytest.mark.parametrize("hw", [(16, 16), (40, 72), (128, 128), (8, 2048)])
def test_warp_is_within_the_derived_bound_of_exact_bilinear(hw):
    """Each source coordinate is off by at most 1 / 64 (the rounding to 1 / 32 pixel) plus 2 x 0.5 / 1024 (the two table roundings):
    17 / 1024; bilinear interpolation is Lipschitz in x with the largest horizontal neighbour difference near the point, and in y
    with the vertical one.  Observed: it holds at every pixel with no allowance for float64 rounding; the worst ratio is 0.988."""
    H, W = hw
    rs = np.random.RandomState(H * 7 + W)
    yy, xx = np.mgrid[0:H, 0:W]
    worst = 0.0
    for name, img in (("random", rs.randint(0, 256, (H, W))), ("smooth", (40 + 0.5 * xx + 0.25 * yy).astype(np.int64) % 256)):
        for ang in ANGLES:
            t = fd.rotation_tables(ang, W, H)
            val, Dx, Dy = _exact_bilinear(img, t.matrix)
            err = np.abs(fd.warp_affine_linear(img, t) / 1024.0 - val)
            bound = (17.0 / 1024.0) * (Dx + Dy)
            assert (err <= bound).all(), (name, ang, float(err.max()), float((err - bound).max()))
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print("worst |S / 1024 - exact| / bound at %d x %d: %.3f" % (H, W, worst))


def test_a_bright_pixel_lands_where_its_landmark_lands():
    for (x, y), ang in (((90, 40), -5), ((90, 40), 4), ((20, 100), 3), ((64, 64), -2)):
        img = np.zeros((128, 128), dtype=np.uint8)
        img[y, x] = 255
        S = fd.warp_affine_linear(img, fd.rotation_tables(ang, 128, 128))
        ys, xs = np.nonzero(S)
        w = S[ys, xs].astype(np.float64)
        centroid = np.array([(xs * w).sum() / w.sum(), (ys * w).sum() / w.sum()])
        lm = fd.rotate_landmarks(np.array([[x, y]], dtype=np.float32), ang, 128, truncate=False)[0]
        assert np.abs(centroid - lm).max() <= 0.1, (x, y, ang, centroid, lm)


def _reference_landmarks(row, ang, load_size):
    """face_dataset.py:122-129 and :82-83, element by element in explicit float32 steps."""
    f32 = np.float32
    lm_aug = np.asarray(row).astype("float32")
    h = f32(load_size // 2)
    arc = -ang * np.pi / 180.0
    c, s = f32(np.cos(arc)), f32(np.sin(arc))
    out = []
    with np.errstate(over="ignore"):
        for x, y in lm_aug:
            x0, y0 = f32(x - h), f32(y - h)
            xr = f32(f32(f32(x0 * c) - f32(y0 * s)) + h)
            yr = f32(f32(f32(x0 * s) + f32(y0 * c)) + h)
            out.append([min(max(xr, f32(0)), f32(load_size)), min(max(yr, f32(0)), f32(load_size))])
    clipped = np.array(out, dtype=np.float32)
    return clipped, torch.clamp(torch.from_numpy(clipped).long(), 0, load_size - 1).numpy()


def test_rotate_landmarks_is_the_reference_chain_in_float32(s16):
    c = fc.case("s16")
    rows = [r for d in ("lm_S", "lm_F") for r in c["lm_dicts"][d].values()]
    assert any((np.asarray(r) < 0).any() and (np.asarray(r) > 127).any() and (np.abs(np.asarray(r)) == 1e6).any() for r in rows)
    for row in rows:
        for flipped in (row, np.hstack((127 - row[:, 0:1], row[:, 1:2]))):
            for ang in ANGLES:
                clipped, final = _reference_landmarks(flipped, ang, 16)
                raw = flipped.astype("float32")
                got = fd.rotate_landmarks(raw, ang, 16, truncate=False)
                assert got.dtype == np.float32 and np.array_equal(got, clipped), ang
                got = fd.rotate_landmarks(raw, ang, 16)
                assert got.dtype == np.int64 and np.array_equal(got, final) and got.min() >= 0 and got.max() <= 15, ang
    with pytest.raises(ValueError):
        fd.rotate_landmarks(np.zeros((3, 2)), 1, 16)          # float64: the chain is defined on the float32 row
    # the raw tables of the store are those rows
    k = s16.host.t["pair_lm"][0, 0].item()
    first = c["lm_dicts"]["lm_S"][fc.key(c["names"][0])]
    assert torch.equal(s16.t["lm_raw"][k], torch.from_numpy(first.astype("float32")))
    assert torch.equal(s16.t["lm_raw_flip"][k], torch.from_numpy(np.hstack((127 - first[:, 0:1], first[:, 1:2])).astype("float32")))
    assert s16.t["lm_raw"].shape == s16.t["lm"].shape and s16.t["lm_raw"].dtype == torch.float32


def test_landmarks_at_angle_zero_are_todays():
    """Integral and half-integral landmarks (exact in float32, and so is x - h + h): angle 0 changes nothing."""
    c = fc.synthetic(3, 8, 8, 40, seed=2)
    assert all((np.asarray(v) == np.trunc(v)).all() for v in c["lm_dicts"]["lm_S"].values())          # integral rows as they come ...
    stores = [_store(c, rotation=True)]
    half = dict(c, lm_dicts=dict(c["lm_dicts"], lm_S={k: np.asarray(v) + 0.5 for k, v in c["lm_dicts"]["lm_S"].items()}))
    stores.append(_store(half, rotation=True))                                                           # ... and half-integral ones
    for store, lm in zip(stores, (c["lm_dicts"]["lm_S"], half["lm_dicts"]["lm_S"])):
        assert any((np.asarray(v) < 0).any() and (np.asarray(v) > 127).any() for v in lm.values())
        for i in range(len(store)):          # unflipped and flipped (127 - x) items
            assert torch.equal(store.host_item(i, 0)["lm_S"], store.host_item(i)["lm_S"]), i
    # the function itself, on rows through the whole range and their flips, for two image sizes
    for load_size in (128, 16):
        for offset in (0.0, 0.5):
            row = np.stack((np.arange(-6.0, 135.0) + offset, np.arange(134.0, -7.0, -1.0) + offset), axis=1)
            for r in (row, np.hstack((127 - row[:, 0:1], row[:, 1:2]))):
                want = torch.clamp(torch.from_numpy(r.copy()).long(), 0, load_size - 1).numpy()
                assert np.array_equal(fd.rotate_landmarks(r.astype("float32"), 0, load_size), want), (load_size, offset)


def test_host_item_changes_the_source_side_only(s16):
    plain = _store(fc.case("s16"))
    for i in range(len(s16)):
        base = plain.host_item(i)
        for ang in (-5, 0, 4):
            item = s16.host_item(i, ang)
            assert set(item) == set(base) and item["input_path"] == base["input_path"]
            for k in ("img_F", "mask_F", "lm_F", "gate"):
                assert item[k].dtype == base[k].dtype and torch.equal(item[k], base[k]), (i, ang, k)
            for k in ("img_S", "mask_S", "lm_S"):
                assert item[k].dtype == base[k].dtype and item[k].shape == base[k].shape, (i, ang, k)
            assert set(item["mask_S"].unique().tolist()) <= {0.0, 1.0}
        zero = s16.host_item(i, 0)
        assert torch.equal(zero["img_S"], base["img_S"])
        assert torch.equal(zero["mask_S"], (base["mask_S"] > 0).float())
        assert not torch.equal(s16.host_item(i, 4)["img_S"], base["img_S"])
    # the flip comes first: item P + i is the rotation of the mirrored image
    c = fc.case("s16")
    P = s16.n_pairs
    S = fd.warp_affine_linear(c["images"][0][:, ::-1], fd.rotation_tables(3, 16, 16))
    want = torch.from_numpy((S / 1024.0).astype("float32").transpose(2, 0, 1)).div(255)
    assert torch.equal(s16.host_item(P, 3)["img_S"], want)
    with pytest.raises(ValueError, match="whole degrees"):
        s16.host_item(0, 0.5)
    batch = s16.host_batch([0, P + 1, 3], [4, -5, 0])
    for j, (i, ang) in enumerate(((0, 4), (P + 1, -5), (3, 0))):
        item = s16.host_item(i, ang)
        assert all(torch.equal(batch[k][j], item[k]) for k in fd.TRAIN_KEYS) and batch["input_path"][j] == item["input_path"]


def test_loader_draws_and_batches(s16):
    big = _store(fc.synthetic(64, 8, 8, 2, seed=4), rotation=True)          # 256 items: a long epoch
    for rotation, lo, hi in ((True, -5, 5), ((-3, 9), -3, 9)):
        loader = fd.FaceLoader(big, 32, seed=7, rotation=rotation)
        plain = fd.FaceLoader(big, 32, seed=7)
        for epoch in (0, 1):
            perm, angles = loader.draws(epoch)
            assert torch.equal(loader.permutation(epoch), plain.permutation(epoch)) and torch.equal(perm, plain.permutation(epoch))
            assert perm.dtype == torch.int32 and angles.shape == (256,)
            assert sorted(set(angles.tolist())) == list(range(lo, hi))          # inside [lo, hi), every value taken
            again = fd.FaceLoader(big, 32, seed=7, rotation=rotation).draws(epoch)
            assert torch.equal(again[0], perm) and torch.equal(again[1], angles)
        assert not torch.equal(loader.draws(0)[1], loader.draws(1)[1])
        assert plain.draws(0)[1] is None
    loader = fd.FaceLoader(s16, 4, seed=5, rotation=True)
    P = s16.n_pairs
    for epoch in (0, 1):
        batches = list(loader)
        perm, angles = loader.draws(epoch)
        assert [b.batch_weight for b in batches] == [4, 4, 2]
        for step, b in enumerate(batches):
            idx, ang = perm[4 * step:4 * step + 4].tolist(), angles[4 * step:4 * step + 4].tolist()
            want = s16.host_batch(idx, ang)
            assert b.input_path == want.pop("input_path") == [s16.names[i % P] for i in idx]
            assert set(b) == set(want) == set(fd.TRAIN_KEYS) and all(torch.equal(b[k], want[k]) for k in want)
            assert b.invalid.tolist() == [0] * len(idx)
    assert loader.epoch == 2


def test_refusals_and_storage(tmp_path, s16):
    c = fc.case("s16")
    plain = _store(c)
    assert s16.can_rotate and not plain.can_rotate and "lm_raw" not in plain.t
    with pytest.raises(ValueError, match="rotation=True"):
        fd.FaceLoader(plain, 2, rotation=True)
    with pytest.raises(ValueError, match="rotation=True"):
        plain.host_item(0, 1)
    test_store = fd.FaceStore.from_arrays(c["images"], None, c["names"], isval=True, load_size=16)
    with pytest.raises(ValueError):
        fd.FaceLoader(test_store, 2, rotation=True)
    with pytest.raises(ValueError):
        fd.FaceStore.from_arrays(c["images"], None, c["names"], isval=True, load_size=16, rotation=True)
    for rng in ((0, 0), (3, 2), (-40, 25)):          # empty, reversed, more than 64 angles
        with pytest.raises(ValueError):
            fd.FaceLoader(s16, 2, rotation=rng)
    assert fd.FaceLoader(s16, 2, rotation=(-32, 32)).rotation.xtab.shape == (64, 2, 16)
    assert fd.FaceLoader(s16, 2, rotation=False).rotation is None and fd.FaceLoader(s16, 2).rotation is None
    for bad in (float("nan"), float("inf"), 1e39):          # (1e39 is not finite in float32)
        lm = {k: {n: np.array(v, dtype=np.float64) for n, v in d.items()} for k, d in c["lm_dicts"].items()}
        lm["lm_F"][fc.key(c["names"][1])][4, 1] = bad
        with pytest.raises(ValueError, match="finite"):
            fd.FaceStore.from_arrays(c["images"], c["masks"], c["names"], lm, load_size=16, rotation=True)
    # aug=True keeps meaning the reference's bytes, certified: it still raises, and says where to go
    with pytest.raises(NotImplementedError, match="warpAffine.*rotation=True"):
        fd.FaceStore.from_arrays(c["images"], c["masks"], c["names"], c["lm_dicts"], load_size=16, aug=True)
    # save -> load carries the raw tables; a file without them loads as before and cannot rotate
    path, old = str(tmp_path / "rot.npz"), str(tmp_path / "old.npz")
    s16.save(path)
    plain.save(old)
    back, back_old = fd.FaceStore.load(path), fd.FaceStore.load(old)
    assert back.can_rotate and set(back.t) == set(s16.t)
    for k in ("lm_raw", "lm_raw_flip"):
        assert back.t[k].dtype == torch.float32 and torch.equal(back.t[k], s16.t[k])
    idx, ang = list(range(len(s16))), [ANGLES[i % 10] for i in range(len(s16))]
    want, got = s16.host_batch(idx, ang), back.host_batch(idx, ang)
    assert all(torch.equal(got[k], want[k]) for k in fd.TRAIN_KEYS)
    assert not back_old.can_rotate and set(back_old.t) == set(plain.t)
    assert all(torch.equal(back_old.host_batch(idx)[k], plain.host_batch(idx)[k]) for k in fd.TRAIN_KEYS)
    with pytest.raises(ValueError, match="rotation=True"):
        fd.FaceLoader(back_old, 2, rotation=True)


def test_directory_store_with_rotation(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    c = fc.case("s16")
    base = tmp_path / "multipie" / "train"
    (base / "images").mkdir(parents=True)
    (base / "masks").mkdir()
    for i, n in enumerate(c["names"]):
        Image.fromarray(c["images"][i], "RGB").save(str(base / "images" / n))
        Image.fromarray(c["masks"][i], "L").save(str(base / "masks" / n))
    np.save(str(base / "landmarks.npy"), c["lm_dicts"], allow_pickle=True)
    got = fd.FaceStore.from_directory(str(tmp_path), "multipie", load_size=16, threads=2, rotation=True)
    assert got.can_rotate and not fd.FaceStore.from_directory(str(tmp_path), "multipie", load_size=16, threads=2).can_rotate
    order = sorted(range(len(c["names"])), key=lambda i: c["names"][i])
    want = fd.FaceStore.from_arrays(c["images"][order], c["masks"][order], [c["names"][i] for i in order], c["lm_dicts"], load_size=16,
                                    rotation=True)
    a, b = got.host_batch([0, 7], [3, -4]), want.host_batch([0, 7], [3, -4])
    assert all(torch.equal(a[k], b[k]) for k in fd.TRAIN_KEYS)


def test_cpu_tensors_are_refused_by_the_op(s16):
    from ffwm_amd import ops
    t, rot = s16.t, s16.rotation(-5, 5)
    with pytest.raises(NotImplementedError):
        ops.face_batch_aug(t["images"], t["pairs"], torch.zeros(1, dtype=torch.int32), t["masks"], t["pair_lm"], t["lm"], t["lm_flip"],
                           t["gate"], t["lm_raw"], t["lm_raw_flip"], torch.zeros(1, dtype=torch.int32), rot.xtab, rot.ytab, rot.cs, 16)
    assert rot.xtab.dtype == rot.ytab.dtype == torch.int32 and rot.cs.dtype == torch.float32
    assert rot.xtab.shape == (10, 2, 16) and rot.ytab.shape == (10, 2, 16) and rot.cs.shape == (10, 2)
    assert rot.slots([-5, 4, 0]).tolist() == [0, 9, 5] and rot.slots(torch.tensor([1])).dtype == torch.int32
    with pytest.raises(ValueError):
        rot.slots([5])
    assert s16.rotation(-5, 5) is rot
    for k in range(12):          # ever new ranges do not pile up table sets
        s16.rotation(-k, k + 1)
    assert len(s16._rotations) == fd._ROTATIONS_KEPT == 8 and (-11, 12) in s16._rotations and (-3, 4) not in s16._rotations
    with pytest.raises(ValueError, match="load_size"):
        s16.batch_rotated([0], [0], fd.FaceRotation(-5, 5, 16, 16, 128))


def test_entry_point_refuses_bad_arguments_before_any_launch():
    from ffwm_amd import build, _lib
    build.build()
    lib = _lib.load()
    assert hasattr(lib, "ffwm_face_batch_aug") and "ffwm_face_batch_aug" in _lib.EXPORTS and _lib.ABI_VERSION == 5
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(images=p, masks=p, pairs=p, pair_lm=p, lm=p, lm_flip=p, gate=p, index=p, lm_raw=p, lm_raw_flip=p, slot=p, xtab=p,
                ytab=p, cs=p, img_S=p, img_F=p, mask_S=p, mask_F=p, lm_S=p, lm_F=p, gate_out=p, invalid=p, N=4, H=16, W=16, P=4, K=8,
                KG=4, L=9, B=2, A=10, load_size=16, train=1)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ffwm_face_batch_aug(*[a[k] for k in good], None)

    for k in [k for k, v in good.items() if v is p]:
        assert call(**{k: None}) == -1 and b"NULL" in lib.ffwm_last_error(), k
    for k in ("N", "H", "W", "P", "K", "KG", "L", "B", "load_size"):
        for v in (0, -1):
            assert call(**{k: v}) == -1 and b"positive" in lib.ffwm_last_error(), (k, v)
    for v in (0, -1, 65):
        assert call(A=v) == -1 and b"1 to 64" in lib.ffwm_last_error(), v
    for v in (0, 2, -1):
        assert call(train=v) == -1 and b"train" in lib.ffwm_last_error(), v
    assert call(W=8193) == -3 and call(H=8193) == -3 and b"8192" in lib.ffwm_last_error()
    assert call(B=65536) == -3 and call(L=(1 << 20) + 1) == -3 and call(N=1 << 31) == -3 and call(P=1 << 30) == -3
    assert call(load_size=(1 << 24) + 1) == -3


def test_against_opencv_where_its_output_is_recorded(s16):
    """tests/golden/make_face_aug_golden.py records what cv2.warpAffine gives for the s16 images (float32, as --preload holds them);
    the file can only be made where OpenCV is installed, which it was not when this was written."""
    path = os.path.join(HERE, "golden", "cv2_warp_affine.npz")
    if not os.path.exists(path):
        pytest.skip("no tests/golden/cv2_warp_affine.npz: it is written where cv2 exists (make_face_aug_golden.py)")
    with np.load(path) as z:
        images, masks, angles = z["images"], z["masks"], z["angles"].tolist()
        for j, ang in enumerate(angles):
            t = fd.rotation_tables(ang, images.shape[2], images.shape[1])
            for i in range(images.shape[0]):
                assert np.array_equal((fd.warp_affine_linear(images[i], t) / 1024.0).astype("float32"), z["warped_images"][j, i]), (ang, i)
                assert np.array_equal((fd.warp_affine_linear(masks[i], t) / 1024.0).astype("float32"), z["warped_masks"][j, i]), (ang, i)

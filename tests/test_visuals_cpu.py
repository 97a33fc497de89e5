"""Result images without a GPU (ffwm_amd/visuals.py, the C entry point's argument checks):
  * the numpy restatements equal the bytes the REFERENCE's util/util.py and util/flow_util.py wrote for the same inputs
    (tests/golden/visuals_ref.npz, made by tests/golden/make_visuals_golden.py under the numpy version it records);
  * to_u8 is numpy's astype(uint8) where that is defined;
  * the routing, the file names, the helpers that build the reference's visual_names;
  * every argument error of ffwm_visuals comes back before a launch;
  * the undecided-pixel condition the GPU test's flow comparison rests on."""
import collections
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

import visual_cases as cases
from ffwm_amd import visuals as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "visuals_ref.npz"))


def _inputs(kind):
    return cases.flow_cases() if kind == "flow" else cases.image_cases()


def _restate(kind, x):
    fn = {"image": V.tensor2im, "mask": V.tensor2mask, "flow": V.tensor2flow}[kind]
    return np.stack([fn(torch.from_numpy(x), idx=i) for i in range(x.shape[0])])


def test_fixture_holds_every_case_and_its_inputs(golden):
    assert str(golden["numpy_version"]).split(".")[0] == "2"          # the float32 / float64 seam of the flow colouring is NumPy 2's
    want = ["%s/%s" % (k, n) for k in ("image", "mask") for n in cases.image_cases()] + ["flow/%s" % n for n in cases.flow_cases()]
    assert sorted(k[4:] for k in golden.files if k.startswith("ref/")) == sorted(want)
    for key in want:
        kind, name = key.split("/")
        x = _inputs(kind)[name]
        if "in/" + key in golden.files:
            assert golden["in/" + key].tobytes() == x.tobytes() and golden["in/" + key].shape == x.shape, key
        else:
            assert str(golden["sha256/" + key]) == hashlib.sha256(x.tobytes()).hexdigest(), key
        assert golden["ref/" + key].shape == (x.shape[0], x.shape[2], x.shape[3], 3) and golden["ref/" + key].dtype == np.uint8


@pytest.mark.parametrize("kind", ["image", "mask"])
def test_image_and_mask_restatements_equal_the_reference(golden, kind):
    """Exact wherever the reference's astype(uint8) is defined (0 <= t < 256, truncation included: -1 < t < 0 is 0).  Outside that
    range the C cast is undefined behaviour and the stated rule is the contract; how often the recorded numpy agreed there is
    printed, not asserted."""
    for name, x in cases.image_cases().items():
        ref, got = golden["ref/%s/%s" % (kind, name)], _restate(kind, x)
        t = x.astype(np.float32)
        if x.shape[1] == 1:
            t = np.tile((t - np.float32(0.5)) * np.float32(2) if kind == "image" else t, (1, 3, 1, 1))
        t = np.transpose(t, (0, 2, 3, 1)) * np.float32(255.0)
        with np.errstate(invalid="ignore"):
            defined = (t > -1) & (t < 256)
        assert defined.any()
        assert (got[defined] == ref[defined]).all(), (kind, name)
        print("%s/%s: %d cells outside [0, 256), the recorded numpy agrees with the stated rule on %d"
              % (kind, name, int((~defined).sum()), int((got[~defined] == ref[~defined]).sum())))


def test_flow_restatement_equals_the_reference(golden):
    for name, f in cases.flow_cases().items():
        ref, got = golden["ref/flow/" + name], _restate("flow", f)
        assert (got == ref).all(), (name, int((got != ref).sum()))
    assert not _restate("flow", cases.flow_cases()["identity_8"]).any()          # no motion: 0 / 0, black
    two = _restate("flow", cases.flow_cases()["two_scales_2x8"])
    assert two[1].any() and (two[0] == two[1]).mean() > 0.5                       # each image normalised by its own maximum


def test_to_u8_is_numpy_cast_where_that_is_defined():
    t = np.concatenate([np.arange(0, 256, dtype=np.float32), np.linspace(0, 255.999, 4001, dtype=np.float32),
                        np.float32([0.0, -0.0, 0.999, 255.0, 255.99998, np.nextafter(np.float32(256), np.float32(0))])])
    assert (V.to_u8(t) == t.astype(np.uint8)).all()
    assert (V.to_u8(t.astype(np.float64)) == t.astype(np.float64).astype(np.uint8)).all()
    # the stated rule outside it: truncate toward zero to int32, low 8 bits; NaN, +-inf, |t| >= 2^31 -> 0
    odd = np.float32([-0.5, -1.0, -63.75, -255.0, -256.0, -257.5, 256.0, 300.9, 76500.0, 2.0 ** 31, -(2.0 ** 31), 2.0 ** 31 - 128, np.nan,
                      np.inf, -np.inf])
    assert V.to_u8(odd).tolist() == [0, 255, 193, 1, 0, 255, 0, 44, 212, 0, 0, 128, 0, 0, 0]
    assert V.to_u8(np.float64(-(2.0 ** 31) + 1)) == 1


def test_color_wheel_follows_the_segment_rule():
    w = V.color_wheel()
    assert w.shape == (55, 3) and w.dtype == np.float64 and (w == np.floor(w)).all() and w.min() == 0 and w.max() == 255
    assert w[0].tolist() == [255, 0, 0] and w[14].tolist() == [255, 238, 0] and w[15].tolist() == [255, 255, 0]
    assert w[21].tolist() == [0, 255, 0] and w[25].tolist() == [0, 255, 255] and w[36].tolist() == [0, 0, 255]
    assert w[49].tolist() == [255, 0, 255] and w[54].tolist() == [255, 0, 43]
    assert (w.max(axis=1) == 255).all()


def test_kind_of_routes_as_the_visualizer_does():
    for label, test_kind, train_kind in (("img_S", V.IMAGE, V.IMAGE), ("fake_F128", V.IMAGE, V.IMAGE), ("mask_S", V.MASK, V.MASK),
                                         ("flow_F128", V.FLOW, V.IMAGE), ("att", V.PALETTE, V.IMAGE),
                                         ("flow_mask", V.MASK, V.MASK),            # 'mask' is asked before 'flow'
                                         ("att_mask", V.PALETTE, V.MASK),          # 'att' before 'mask'
                                         ("flow_att", V.PALETTE, V.IMAGE), ("pattern", V.PALETTE, V.IMAGE)):    # a substring is enough
        assert V.kind_of(label) == V.kind_of(label, test=True) == test_kind, label
        assert V.kind_of(label, test=False) == train_kind, label


def _visuals():
    x, pal = cases.palette_case()
    v = collections.OrderedDict()
    v["img_S"] = torch.from_numpy(cases.image_cases()["rgb_2x3x5x7"])
    v["mask_S"] = torch.from_numpy(cases.image_cases()["gray_2x1x5x7"])
    v["flow_F128"] = torch.from_numpy(cases.flow_cases()["odd_2x5x7"])
    v["att"] = torch.from_numpy(x)
    return v, pal


def test_render_on_cpu_tensors_is_the_restatements():
    v, pal = _visuals()
    r = V.render(v, palette=pal)
    assert list(r) == list(v)
    for label, fn in (("img_S", V.tensor2im), ("mask_S", V.tensor2mask), ("flow_F128", V.tensor2flow)):
        assert r[label].dtype == torch.uint8 and tuple(r[label].shape) == (2, 5, 7, 3)
        for i in range(2):
            assert (r[label][i].numpy() == fn(v[label], idx=i)).all()
    x = v["att"].numpy()
    assert (r["att"].numpy() == pal[(x[:, 0] * np.float32(255.0)).astype(np.uint8)]).all()
    # training-time routing knows masks and images only
    rt = V.render(v, test=False)
    assert (rt["flow_F128"][0].numpy() == V.tensor2im(v["flow_F128"])).all() and (rt["att"][1].numpy() == V.tensor2im(v["att"], idx=1)).all()
    with pytest.raises(ValueError, match="COLORMAP_JET"):
        V.render(v)
    with pytest.raises(ValueError, match="COLORMAP_JET"):
        V.tensor2att(v["att"], None)
    with pytest.raises(ValueError):
        V.tensor2att(v["att"], pal[:, :2])


def test_result_writer_files_decode_to_the_rendered_arrays(tmp_path):
    from PIL import Image
    import ffwm_amd
    assert ffwm_amd.ResultWriter is V.ResultWriter
    v, pal = _visuals()
    w = V.ResultWriter(str(tmp_path / "test" / "multipie"), img_dir=str(tmp_path / "web" / "images"), palette=pal)
    paths = w.save_test(v, ["001_01_01_051_07", "002_01_01_140_07"])
    want = ["%s_%s.png" % (p, label) for p in ("001_01_01_051_07", "002_01_01_140_07") for label in v]
    assert [os.path.basename(p) for p in paths] == want and sorted(os.listdir(w.test_dir)) == sorted(want)
    r = V.render(v, palette=pal)
    for idx, prefix in enumerate(("001_01_01_051_07", "002_01_01_140_07")):
        for label in v:
            img = np.asarray(Image.open(os.path.join(w.test_dir, "%s_%s.png" % (prefix, label))))
            assert img.shape == (5, 7, 3) and (img == r[label][idx].numpy()).all(), (prefix, label)
    assert [os.path.basename(p) for p in w.save_test(v, [None, "x"])] == ["x_%s.png" % label for label in v]    # not in visual_list: skipped
    with pytest.raises(ValueError):
        w.save_test(v, ["only_one"])
    paths = w.save_train(v, 7)
    assert [os.path.basename(p) for p in paths] == ["epoch007_%s.png" % label for label in v]
    rt = V.render(v, test=False)
    for label in v:
        img = np.asarray(Image.open(os.path.join(w.img_dir, "epoch007_%s.png" % label)))
        assert (img == rt[label][0].numpy()).all(), label


def test_from_result_and_train_visuals_build_the_reference_names():
    R = collections.namedtuple("FrontalizerResult", "fake_F128 fake_F64 fake_F32 img_S_warp att flows")
    t = {k: torch.zeros(1) + i for i, k in enumerate(("fake_F128", "fake_F64", "fake_F32", "img_S_warp", "att", "f128", "f64", "f32",
                                                       "img_S", "img_F"))}
    r = R(t["fake_F128"], t["fake_F64"], t["fake_F32"], t["img_S_warp"], t["att"], (t["f128"], t["f64"], t["f32"]))
    v = V.from_result(r, t["img_S"], t["img_F"])
    assert list(v) == ["img_S", "img_F", "fake_F128"] and v["fake_F128"] is t["fake_F128"] and v["img_F"] is t["img_F"]
    v = V.from_result(r, t["img_S"], extra=("img_S_warp", "att", "flow_F128"))
    assert list(v) == ["img_S", "fake_F128", "img_S_warp", "att", "flow_F128"] and v["flow_F128"] is t["f128"] and v["att"] is t["att"]
    with pytest.raises(ValueError):
        V.from_result(r, t["img_S"], extra=("flows",))

    class Trainer(object):
        pass
    tr = Trainer()
    for i, k in enumerate(("fake32", "fake64", "fake128", "img_GF128", "img_S_warp", "img_S_rec")):
        setattr(tr, k, torch.zeros(1) + 10 + i)
    v = V.train_visuals(tr, {"img_S": t["img_S"], "img_F": t["img_F"], "mask_S": None})
    assert list(v) == ["img_S", "img_F", "img_S_warp", "fake_F32", "fake_F64", "fake_F128", "img_S_rec", "img_GF128"]
    assert v["fake_F32"] is tr.fake32 and v["fake_F64"] is tr.fake64 and v["fake_F128"] is tr.fake128 and v["img_GF128"] is tr.img_GF128
    assert vars(tr).keys() == {"fake32", "fake64", "fake128", "img_GF128", "img_S_warp", "img_S_rec"}           # read, not changed


# ------------------------------------------------------------------------------------------------ the C entry point, before any launch
@pytest.fixture(scope="module")
def hiplib():
    from ffwm_amd import build, _lib
    build.build()
    return _lib.load()


def _table(*rows):
    from ffwm_amd import ops
    arr = (ops._VisualItem * max(len(rows), 1))()
    for a, (src, pal, out, kind, B, C, H, W) in zip(arr, rows):
        a.src, a.palette, a.out, a.kind, a.B, a.C, a.H, a.W = src, pal, out, kind, B, C, H, W
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def test_symbol_is_exported_and_the_abi_is_still_5(hiplib):
    from ffwm_amd import _lib
    assert "ffwm_visuals" in _lib.EXPORTS and "ffwm_visuals_workspace_bytes" in _lib.EXPORTS
    assert hasattr(hiplib, "ffwm_visuals") and hasattr(hiplib, "ffwm_visuals_workspace_bytes")
    assert hiplib.ffwm_abi_version() == _lib.ABI_VERSION == 5


def test_argument_errors_are_reported_before_launch(hiplib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    ok = (p, None, p, V.IMAGE, 1, 3, 2, 2)

    def call(rows, n=None, ws=None, ws_bytes=0, dtype=0):
        keep, table = _table(*rows)
        return hiplib.ffwm_visuals(table, len(rows) if n is None else n, ws, ws_bytes, dtype, None)

    assert call([ok], dtype=1) == -2 and call([ok], dtype=7) == -2 and b"float32" in hiplib.ffwm_last_error()
    assert hiplib.ffwm_visuals(None, 1, None, 0, 0, None) == -1 and b"NULL" in hiplib.ffwm_last_error()
    assert call([ok], n=0) == -1 and call([ok], n=-3) == -1
    assert call([ok] * 17) == -1 and b"17 items" in hiplib.ffwm_last_error()
    assert call([(None,) + ok[1:]]) == -1 and b"NULL" in hiplib.ffwm_last_error()
    assert call([ok[:2] + (None,) + ok[3:]]) == -1 and b"NULL" in hiplib.ffwm_last_error()
    assert call([ok, ok[:3] + (4,) + ok[4:]]) == -1 and b"item 1: kind 4" in hiplib.ffwm_last_error()
    assert call([ok[:3] + (-1,) + ok[4:]]) == -1
    for kind, C in ((V.IMAGE, 2), (V.IMAGE, 4), (V.MASK, 2), (V.FLOW, 1), (V.FLOW, 3)):
        assert call([(p, None, p, kind, 1, C, 2, 2)]) == -1 and b"does not take C" in hiplib.ffwm_last_error(), (kind, C)
    for dims in ((0, 3, 2, 2), (1, 0, 2, 2), (1, 3, 0, 2), (1, 3, 2, -1)):
        assert call([(p, None, p, V.IMAGE) + dims]) == -1 and b"non-positive" in hiplib.ffwm_last_error()
    assert call([(p, None, p, V.PALETTE, 1, 1, 2, 2)]) == -1 and b"palette" in hiplib.ffwm_last_error()
    assert call([(p, None, p + 2, V.IMAGE, 1, 3, 2, 2)]) == -1 and b"aligned" in hiplib.ffwm_last_error()
    assert call([(p, None, p, V.IMAGE, 1 << 20, 3, 1 << 6, 1 << 6)]) == -3
    flow = (p, None, p, V.FLOW, 3, 2, 2, 2)
    assert call([ok, flow]) == -1 and b"workspace" in hiplib.ffwm_last_error()                     # missing
    assert call([ok, flow], ws=p, ws_bytes=8) == -1 and b"12 bytes" in hiplib.ffwm_last_error()    # too small: one float per flow image
    keep, table = _table(ok, flow, flow)
    assert hiplib.ffwm_visuals_workspace_bytes(table, 3) == 24 and hiplib.ffwm_visuals_workspace_bytes(table, 1) == 0
    assert hiplib.ffwm_visuals_workspace_bytes(table, 0) == -1 and hiplib.ffwm_visuals_workspace_bytes(None, 1) == -1


def test_ops_visuals_refuses_cpu_tensors_and_bad_tables():
    from ffwm_amd import ops
    assert ops.visuals([]) == []
    with pytest.raises(NotImplementedError):
        ops.visuals([(torch.rand(1, 3, 4, 4), V.IMAGE, None)])


# ------------------------------------------------------------------------------------------------ the undecided-pixel condition
def test_undecided_pixels_are_few_and_one_level_apart():
    """What the GPU test's flow comparison rests on.  The kernel's float64 atan2 is another libm's: where moving arctan2's result by
    +-4 ulp changes no byte of a pixel, a faithful atan2 cannot either (decided); elsewhere the GPU may differ by the step the
    perturbation itself makes.  At most 1 % of an image's pixels may be undecided, and the two perturbed images at most 1 level apart."""
    for name, f in cases.flow_cases().items():
        for idx in range(f.shape[0]):
            _, und, spread = cases.undecided(f, idx)
            print("%s[%d]: %d of %d pixels undecided, perturbed images %d level(s) apart" % (name, idx, int(und.sum()), und.size, spread))
            assert int(und.sum()) * 100 <= und.size, (name, idx, int(und.sum()))
            assert spread <= 1, (name, idx, spread)

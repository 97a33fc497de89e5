"""ffwm_amd/identity_eval.py without a GPU: the torch backend of FoldedLightCNN and FaceIdentifier's input against the reference's
fixtures, the launch plan, the rank-1 meter, and the bound of the centre-face crop (tests/identity_bounds.py) held against ATen's own
fp32 composition and against two wrong variants."""
import copy
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import fill  # noqa: E402
import identity_bounds as ib  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return torch.load(os.path.join(HERE, "golden", "reference_identity.pt"))


@pytest.fixture(scope="module")
def modules_gold():
    return torch.load(os.path.join(HERE, "golden", "reference_modules.pt"))


@pytest.fixture(scope="module")
def filled():
    from ffwm_amd import nets
    from ffwm_amd.identity_eval import FoldedLightCNN
    net = fill.fill_module(nets.LightCNN29()).eval()
    return net, FoldedLightCNN(net)


def _close(got, ref, tol):
    d = (got - ref).abs().max().item()
    assert d <= tol, (d, tol)
    return d


def test_torch_backend_against_the_module_and_the_fixture(filled, modules_gold):
    """The tolerance tests/test_nets_golden.py::test_discriminator_and_lightcnn holds the module path to, against the reference's
    fixture; float64 against the float64 module."""
    from ffwm_amd.identity_eval import FoldedLightCNN
    net, folded = filled
    assert folded.backend == "torch"
    x = fill.image(2, 1, 128, 128, "lightcnn_in")
    fc, pool = folded(x)
    g = modules_gold["lightcnn_eval"]
    assert fc.shape == (2, 256) and pool.shape == (2, 128, 8, 8)
    _close(fc, g["fc"], 1e-4 * (1 + g["fc"].abs().max().item()))
    _close(pool[..., ::2, ::2], g["pool_s2"], 1e-4 * (1 + g["pool_s2"].abs().max().item()))
    assert abs(pool.double().sum().item() - g["pool_sum"].item()) <= 1e-4 * pool.double().abs().sum().item()
    net64 = copy.deepcopy(net).double()
    with torch.no_grad():
        _, fc64, pool64 = net64(x.double())
    fc_d, pool_d = FoldedLightCNN(net64)(x.double())
    _close(fc_d, fc64, 1e-9 * fc64.abs().max().item())
    _close(pool_d, pool64, 1e-9 * pool64.abs().max().item())


def test_the_classifier_is_not_kept(filled):
    net, folded = filled
    held = sum(t.numel() for L in folded.layers.values() for t in (L.w, L.b)) + folded.fc_w.numel() + folded.fc_b.numel()
    assert held == sum(p.numel() for n, p in net.named_parameters() if not n.startswith("fc2."))
    assert net.fc2.weight.numel() > 20e6          # the 79 077-way classifier: 81 MB that inference never reads
    with pytest.raises(ValueError):
        from ffwm_amd.identity_eval import FoldedLightCNN
        FoldedLightCNN(copy.deepcopy(net).train())


def test_plan_one_tail_per_convolution(filled):
    """Every convolution of the network (29: the stem, 10 residual blocks of two, 4 groups of two -- lightcnn/light_cnn.py:82-99) is
    followed by exactly one mfm_tail; no separate add or pool exists as a kind; the pools of a 120 x 120 input are ceil-mode."""
    import torch.nn as nn
    from ffwm_amd import identity_eval
    net, folded = filled
    n_conv = sum(isinstance(m, nn.Conv2d) for m in net.modules())
    assert n_conv == 29 == len(folded.layer_names())
    plan = folded.plan(1, 128, 128)
    kinds = [k for _, k in plan]
    assert kinds.count("mfm_tail") == n_conv
    assert set(kinds) <= set(identity_eval.KINDS) and not any("add" in k or "pool" in k for k in identity_eval.KINDS)
    assert len(plan) == 2 * n_conv + 2 and plan[-2:] == [("fc", "linear"), ("fc", "mfm")]
    for i in range(n_conv):
        assert plan[2 * i][0] == plan[2 * i + 1][0] == folded.layer_names()[i]
        assert plan[2 * i][1] in ("winograd", "conv_mfma", "vendor_conv") and plan[2 * i + 1][1] == "mfm_tail"
    assert plan[0] == ("conv1", "vendor_conv")                                  # the 5 x 5 stem
    assert all(k == "vendor_conv" for n, k in plan[::2] if n.endswith("conv_a"))    # the 1 x 1 layers
    # 120 -> 60 -> 30 -> 15 -> 8: the last pool is the ceil-mode one; the plan's own shape walk ends at fc's 8 x 8 x 128 inputs
    assert len(folded.plan(1, 120, 120)) == len(plan)
    fc, pool = folded(fill.image(1, 1, 120, 120, "lightcnn_120"))
    assert pool.shape == (1, 128, 8, 8) and fc.shape == (1, 256)
    with pytest.raises(ValueError):
        folded.plan(1, 96, 96)                                                  # 6 x 6 x 128 does not fit fc


def test_crop_grid_is_the_reference_grid(modules_gold):
    from ffwm_amd.identity_eval import crop_grid
    assert torch.equal(crop_grid(2), modules_gold["identity_grid98"])


def test_cropped_input_and_feature_against_the_fixture(filled, gold):
    from ffwm_amd.identity_eval import torch_identity_input
    _, folded = filled
    img = fill.image(2, 3, 128, 128, "ident_img")
    cropped = torch_identity_input(img, crop=True)
    _close(cropped, gold["cropped"], 1e-6)
    fc, _ = folded(cropped)
    _close(fc, gold["fc_cropped"], 1e-4 * (1 + gold["fc_cropped"].abs().max().item()))
    assert torch.equal(torch_identity_input(img, crop=False), img.mean(1, keepdim=True))
    with pytest.raises(ValueError):
        torch_identity_input(torch.zeros(1, 3, 64, 64), crop=True)


def test_crop_bound_holds_for_aten_and_breaks_for_wrong_variants(gold, modules_gold):
    """The bound of the GPU test: met by ATen's fp32 composition fed the stored fp32 grid and by the fixture tensor; the
    align_corners=True resize and a crop centred on row 64 instead of 77 miss it by a wide factor."""
    assert ib.crop_taps_inside()
    ys, xs = ib.crop_coordinates()
    assert ys[0] == 27.5 and xs[0] == 14.5 and ys[-1] == 125.5 and xs[-1] == 112.5
    img = fill.image(2, 3, 128, 128, "ident_img")
    ref, bound = ib.crop_bound(img)
    # the float64 formula is the float64 ATen composition
    from ffwm_amd.identity_eval import crop_grid
    grid64 = crop_grid(2, dtype=torch.float64)
    assert (grid64 - modules_gold["identity_grid98"].double()).abs().max().item() <= 2.0 ** -23          # the stored fp32 grid, rounded
    aten64 = F.interpolate(F.grid_sample(img.double().mean(1, keepdim=True), grid64.permute(0, 2, 3, 1), mode="bilinear",
                                         padding_mode="zeros", align_corners=False), (128, 128), mode="bilinear")
    assert (aten64 - ref).abs().max().item() <= 1e-12
    gray = img.mean(1, keepdim=True)
    aten32 = F.interpolate(F.grid_sample(gray, modules_gold["identity_grid98"].permute(0, 2, 3, 1), mode="bilinear", padding_mode="zeros",
                                         align_corners=False), (128, 128), mode="bilinear")
    r_aten, r_fix = ib.worst_ratio(aten32, ref, bound), ib.worst_ratio(gold["cropped"], ref, bound)
    wrong_resize = ib.crop_reference(img, align_corners=True)
    wrong_centre = ib.crop_reference(img, row_origin=ib.COL_ORIGIN)
    r_resize, r_centre = ib.worst_ratio(wrong_resize, ref, bound), ib.worst_ratio(wrong_centre, ref, bound)
    print("crop bound: ATen fp32 %.3g, fixture %.3g, align_corners=True %.3g, row centre 64 %.3g (error / bound)" % (
        r_aten, r_fix, r_resize, r_centre))
    assert r_aten <= 1.0 and r_fix <= 1.0
    assert r_resize >= 100.0 and r_centre >= 100.0
    # the gray bound likewise: ATen's fp32 mean
    gref, gbound = ib.gray_bound(img)
    assert ib.worst_ratio(gray, gref, gbound) <= 1.0


def test_rank_meter_equals_the_reference_meter(gold):
    from ffwm_amd import RankMeter
    from ffwm_amd.identity_eval import torch_cosine_topk
    names, keys, probe, gallery = ib.meter_case()
    assert names == gold["meter"]["names"] and keys == gold["meter"]["keys"] and len(names) == 24 and len(keys) == 20
    assert sorted(set(os.path.basename(n).split("_")[3] for n in names)) == sorted(ib.CAMERAS)
    ref, _ = ib.cosine_reference(probe, gallery)
    assert ib.rank_gaps(ref, 10) > ib.RANK_GAP                  # no ties among the leaders: the fixture does not hang on a tie rule
    sim, idx = torch_cosine_topk(probe, gallery, 10)
    assert idx.shape == (24, 10) and idx.dtype == torch.int32
    assert torch.equal(idx.long(), torch.topk(ref, 10, dim=1)[1])
    meter = RankMeter()
    meter.update(idx, names, keys, topk=1)
    assert meter.stat_dict == gold["meter"]["stat_dict"]
    assert str(meter) == gold["meter"]["str"]
    wrong = sum(v["all"] - v["correct"] for v in meter.stat_dict.values())
    assert 0 < wrong < 24                                       # the case has hits and misses
    # cameras never seen: their degree is left out (the reference raises KeyError)
    part = RankMeter()
    part.update(idx[:2], names[:2], keys)
    text = str(part)
    assert text.count("\n") == 2 + 1 + 1 and "15: [" in text and "30: [" not in text
    part.reset()
    assert part.stat_dict == {} and str(part) == "\n"
    with pytest.raises(ValueError):
        part.update(idx[:2], names[:3], keys)


def test_tie_and_k_rules_on_hand_made_rows():
    from ffwm_amd.identity_eval import torch_cosine_topk, RankMeter
    e = torch.eye(4)
    gallery = torch.stack([e[1], e[0], e[0], e[2], 2 * e[0]])           # rows 1, 2 and 4 are one direction
    probe = torch.stack([e[0], e[2] + 0.5 * e[1]])
    sim, idx = torch_cosine_topk(probe, gallery, 5)
    assert idx[0].tolist() == [1, 2, 4, 0, 3]                           # equal similarity: the lower index first
    assert idx[1].tolist()[:2] == [3, 0]
    assert torch.all(sim[:, :-1] >= sim[:, 1:])
    # k = min(max(10, topk), G), as AverageMeter.update takes it
    from ffwm_amd.identity_eval import FaceIdentifier
    ident = FaceIdentifier.__new__(FaceIdentifier)
    for topk, G, want in ((1, 250, 10), (1, 5, 5), (20, 250, 20), (20, 12, 12)):
        ident.topk, ident.gallery_features = topk, torch.zeros(G, 256)
        assert ident.k == want
    ident.gallery_features = None
    assert ident.k is None
    # top-k counting: a hit anywhere in the first `topk`
    m = RankMeter()
    m.update([[1, 0, 2]], ["a/002_01_01_050_00.png"], ["001", "002", "003"], topk=1)
    m.update([[1, 0, 2]], ["001_01_01_050_00.png"], ["001", "002", "003"], topk=1)
    m.update([[1, 0, 2]], ["001_01_01_050_00.png"], ["001", "002", "003"], topk=2)
    assert m.stat_dict == {"050": {"correct": 2, "all": 3}}


def test_new_symbols_are_declared_and_bound():
    from ffwm_amd import _lib
    text = open(os.path.join(os.path.dirname(HERE), "include", "ffwm_hip.h")).read()
    for name in ("ffwm_mfm_tail_forward", "ffwm_identity_input", "ffwm_cosine_topk", "ffwm_cosine_topk_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 5


def test_argument_errors_come_before_any_launch():
    """No device here: every refusal below is decided on the host."""
    import ctypes
    from ffwm_amd import build, _lib
    build.build()
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.ffwm_mfm_tail_forward(None, None, None, None, 1, 1, 2, 2, 0, 0, None) == -1 and b"NULL" in lib.ffwm_last_error()
    assert lib.ffwm_mfm_tail_forward(p, None, None, p, 1, 1, 2, 2, 0, 1, None) == -2
    assert lib.ffwm_mfm_tail_forward(p, None, None, p, 1, 1, 2, 2, 2, 0, None) == -1 and b"pool" in lib.ffwm_last_error()
    assert lib.ffwm_mfm_tail_forward(p, None, None, p, 1, 0, 2, 2, 0, 0, None) == -1
    assert lib.ffwm_identity_input(p, p, 1, 3, 64, 64, 1, 0, None) == -1 and b"128" in lib.ffwm_last_error()
    assert lib.ffwm_identity_input(p, p, 1, 0, 4, 4, 0, 0, None) == -1
    assert lib.ffwm_identity_input(p, p, 1, 3, 4, 4, 0, 1, None) == -2
    assert lib.ffwm_cosine_topk(p, p, p, p, 1, 4, 8, 5, p, 1 << 20, 0, None) == -1 and b"k must" in lib.ffwm_last_error()
    assert lib.ffwm_cosine_topk(p, p, p, p, 1, 64, 8, 33, p, 1 << 20, 0, None) == -1
    assert lib.ffwm_cosine_topk(p, p, p, p, 1, 4, 1025, 1, p, 1 << 20, 0, None) == -1 and b"1024" in lib.ffwm_last_error()
    assert lib.ffwm_cosine_topk(p, p, p, p, 1, 4, 8, 1, p, 0, 0, None) == -1 and b"workspace" in lib.ffwm_last_error()
    assert lib.ffwm_cosine_topk(p, p, p, p, 1, 4, 8, 1, p, 1 << 20, 1, None) == -2
    # similarities [B, G] float32, and k candidate keys per (probe, 2048-row segment) once there is more than one segment
    assert lib.ffwm_cosine_topk_workspace_bytes(1, 250, 256, 10) == 1008
    assert lib.ffwm_cosine_topk_workspace_bytes(64, 65536, 256, 10) == 64 * 65536 * 4 + 64 * 32 * 10 * 8
    assert lib.ffwm_cosine_topk_workspace_bytes(1, 4, 8, 5) == 0


def test_lazy_exports():
    import ffwm_amd
    from ffwm_amd import identity_eval
    for name in ("FaceIdentifier", "FoldedLightCNN", "IdentityResult", "RankMeter"):
        assert getattr(ffwm_amd, name) is getattr(identity_eval, name)
        assert name in ffwm_amd.__doc__
    assert ffwm_amd.IdentityResult._fields == ("frontal", "feature", "top_sim", "top_idx")


def test_face_identifier_torch_backend_and_the_gpu_case_inputs(tmp_path):
    """FaceIdentifier on the CPU (torch backend) from checkpoints in the reference's layout; the inputs of the GPU test qualify: at
    least 90 % of the probe rows have rank gaps above RANK_GAP among their first k similarities."""
    import test_trainer_cpu as T
    import ffwm_amd
    gold, ckpt_dir = T._eval_golden()
    ep = T._prepare_reference_checkpoints(tmp_path, gold, ckpt_dir)
    light = ib.saved_lightcnn(os.path.join(str(tmp_path), "lightcnn.pth"))
    ident = ffwm_amd.FaceIdentifier.from_checkpoints(str(tmp_path), ep, light, ngf=4, device="cpu", graph=False)
    assert ident.backend == "torch" and ident.k is None
    keys, gallery, probes, _ = ib.identifier_case()
    r = ident(probes[:2])
    assert r.top_sim is None and r.top_idx is None and r.feature.shape == (2, 256)
    print("fake_F128", T._packed_close(r.frontal.fake_F128, gold["test_forward"]["fake_F128"], 1e-4))
    ident.set_gallery(keys, gallery)
    assert ident.k == 10 and ident.gallery_features.shape == (12, 256) and ident.gallery_keys == keys
    r = ident(probes)
    assert r.top_sim.shape == (4, 10) and r.top_idx.shape == (4, 10) and r.top_idx.dtype == torch.int32
    ok = ib.qualifying_rows(r.top_sim)
    print("rank gaps:", (r.top_sim[:, :-1] - r.top_sim[:, 1:]).min(dim=1)[0].tolist())
    assert ok.float().mean().item() >= 0.9
    # the feature is the reference's composition: gray of fake_F128 through the module
    from ffwm_amd import nets
    net = fill.fill_module(nets.LightCNN29()).eval()
    with torch.no_grad():
        _, fea, _ = net(torch.mean(r.frontal.fake_F128, dim=(1,), keepdim=True))
    assert torch.equal(fea, r.feature)
    with pytest.raises(ValueError):
        ffwm_amd.FaceIdentifier.from_checkpoints(str(tmp_path), ep, light, ngf=4, device="cpu", graph=True)

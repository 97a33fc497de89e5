"""FoldedFFWM / Frontalizer (ffwm_amd/ffwm_eval.py) without a GPU: the folding algebra through the torch backend against the
reference fixture and a float64 evaluation of the module, the spectral-norm snapshot, the launch plan, checkpoint loading, and the
argument checks of the four entry points of csrc/netg_eval.hip.

Every netG here carries the closed-form weights of tests/golden/fill.py: a default-initialised FFWM(sn=True) overflows in eval mode
(its u / v were never iterated)."""
import copy
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import fill  # noqa: E402
import torch_refs  # noqa: E402

EPS32 = float(torch.finfo(torch.float32).eps)
FEATURES = ["e0", "e1", "e2", "e3", "d0", "d1", "d2", "dres0", "dres1", "dres2"]


def _filled_net():
    from ffwm_amd import nets
    return fill.fill_module(nets.FFWM(sn=True, warp_flipcat=torch_refs.warp_flipcat)).eval()


def _inputs(B=1, S=128):
    img = fill.image(B, 3, S, S, "netG_in")
    flows = [fill.flow_field(B, s, s, "netG_flow%d" % s) for s in (S // 4, S // 2, S)]
    return img, flows


def module_features(net, img, flows):
    """(rec32, rec64, rec128, att), {feature name: output of that submodule} of the MODULE's forward."""
    feats, hooks = {}, []
    for name in FEATURES:
        hooks.append(getattr(net, name).register_forward_hook(lambda m, i, o, name=name: feats.__setitem__(name, o)))
    try:
        with torch.no_grad():
            out = net(img, flow=flows, return_att=True)
    finally:
        for h in hooks:
            h.remove()
    return out, feats


@pytest.fixture(scope="module")
def runs():
    """One folded float32 run and one float64 module run at B = 1, 128 x 128, shared and left unchanged."""
    from ffwm_amd.ffwm_eval import FoldedFFWM
    torch.set_num_threads(8)
    net = _filled_net()
    img, flows = _inputs()
    folded = FoldedFFWM(net, backend="torch")
    r32, r64, r128, att, feats = folded(img, flows, return_att=True, return_features=True)
    net64 = copy.deepcopy(net).double()
    ref_out, ref_feats = module_features(net64, img.double(), [f.double() for f in flows])
    return {"net": net, "folded": folded, "out": (r32, r64, r128, att), "feats": feats, "ref_out": ref_out, "ref_feats": ref_feats}


def test_folded_forward_matches_the_reference_fixture(runs):
    gold = torch.load(os.path.join(HERE, "golden", "reference_modules.pt"))["ffwm_eval"]
    r32, r64, r128, att = runs["out"]
    for got, ref in ((r32, gold["rec32"]), (r64, gold["rec64"]), (r128[..., ::2, ::2], gold["rec128_s2"]), (att[..., ::8, ::8], gold["att_s8"])):
        d = (got - ref).abs().max().item()
        print("fixture: max abs diff %.3e" % d)
        assert d <= 2e-5, d


def test_folded_features_match_the_float64_module(runs):
    """max|diff| <= 1e-4 * max|ref| per tensor: the project's fp32 contract on each tensor's own scale (the filled net's features
    are 0.05-0.2 in magnitude)."""
    pairs = [(n, runs["feats"][n], runs["ref_feats"][n]) for n in FEATURES]
    pairs += [(n, g, r) for n, g, r in zip(("rec32", "rec64", "rec128", "att"), runs["out"], runs["ref_out"])]
    assert sorted(runs["feats"]) == sorted(FEATURES)
    worst = 0.0
    for name, got, ref in pairs:
        assert got.shape == ref.shape, name
        rel = (got.double() - ref).abs().max().item() / ref.abs().max().item()
        print("%-6s rel %.3e" % (name, rel))
        worst = max(worst, rel)
        assert rel <= 1e-4, (name, rel)
    assert worst > 0.0


def _sn_paths(net):
    return sorted(n[:-len(".weight_orig")] for n in net.state_dict() if n.endswith(".weight_orig"))


def test_spectral_norm_snapshot_equals_the_eval_weights(runs):
    """The snapshot (weight_orig / (u . (W v)) from the state dict, float64, rounded once) against the `.weight` the per-layer hooks
    set in an eval forward; a net that went through fuse_spectral_norm gives the same snapshot (same state dict, no forward needed --
    its batched kernel itself runs on the GPU only: tests/test_gpu_frontalizer.py)."""
    from ffwm_amd.ffwm_eval import FoldedFFWM
    from ffwm_amd.spectral_norm import fuse_spectral_norm
    net = copy.deepcopy(runs["net"])
    img, flows = _inputs(1, 32)
    with torch.no_grad():
        net(img, flow=flows)                       # the hooks set `.weight` of every layer
    folded = runs["folded"]
    paths = _sn_paths(net)
    assert len(paths) == 52 and sorted(folded.sn_weights) == paths
    for p in paths:
        w = net.get_submodule(p).weight
        d = (folded.sn_weights[p] - w).abs().max().item()
        assert d <= 2 * EPS32 * w.abs().max().item(), (p, d)
    fused = copy.deepcopy(runs["net"])
    fuse_spectral_norm(fused)
    again = FoldedFFWM(fused, backend="torch")
    for p in paths:
        assert torch.equal(again.sn_weights[p], folded.sn_weights[p]), p
    for name, L in folded.layers.items():
        assert torch.equal(again.layers[name].w, L.w) and (L.b is None or torch.equal(again.layers[name].b, L.b)), name


def test_folded_refuses_a_training_network():
    from ffwm_amd import nets
    from ffwm_amd.ffwm_eval import FoldedFFWM
    net = nets.FFWM(sn=True, warp_flipcat=torch_refs.warp_flipcat)
    with pytest.raises(ValueError):
        FoldedFFWM(net, backend="torch")
    with pytest.raises(NotImplementedError):
        FoldedFFWM(net.eval(), backend="hip")          # a CPU network
    with pytest.raises(ValueError):
        FoldedFFWM(net.eval(), backend="torch", graph=True)


@pytest.mark.parametrize("shape", [(8, 128, 128), (1, 32, 32)])
def test_launch_plan(runs, shape):
    from ffwm_amd import build, ffwm_eval
    build.build()                                   # the route predicates ask the library how it would cut a Winograd call
    plan = runs["folded"].plan(*shape)
    kinds = [k for _, k in plan]
    assert set(kinds) <= set(ffwm_eval.KINDS)
    assert not any("bn" in k or "batch" in k or k in ("lrelu", "act", "sigmoid", "cat") for k in kinds)
    tails = [n for n, k in plan if k in ("add_act", "gate")]
    blocks = ["e0.2", "e1.3", "e2.3", "e3.3"] + ["dres%d.%d" % (i, j) for i in range(3) for j in range(2)] + ["att%d.1" % i for i in range(3)]
    assert sorted(tails) == sorted(blocks) and len(tails) == 13
    assert sorted(n for n, k in plan if k == "gate") == ["att0.1", "att1.1", "att2.1"]
    assert sorted(n for n, k in plan if k == "shuffle_bias_act") == ["d0", "d1", "d2"]
    assert sorted(n for n, k in plan if k == "image_head") == ["rec0.0", "rec1.0", "rec2.0"]
    assert kinds.count("upsample2x") == 2 and kinds.count("warp_multi") == 1
    for i, (name, kind) in enumerate(plan):
        if kind == "bias_act":
            assert i > 0 and plan[i - 1] == (name, "vendor_conv"), (i, name)
    # every convolution of the network exactly once: 52 spectrally normalised layers, three of them the image heads
    convs = [n for n, k in plan if k in ("winograd", "conv_mfma", "vendor_conv")]
    assert sorted(convs + ["rec%d.0" % i for i in range(3)]) == _sn_paths(runs["net"])
    assert ("e0.0", "vendor_conv") in plan and all(("%s.input" % b, "vendor_conv") in plan for b in blocks)


def test_launch_plan_routes_follow_the_plane_size(runs):
    from ffwm_amd import build
    build.build()
    big, small = dict(runs["folded"].plan(8, 128, 128)), dict(runs["folded"].plan(1, 32, 32))
    assert big["dres2.0.blocks.0"] == "winograd" and big["e1.0"] == "conv_mfma" and big["e3.3.blocks.0"] == "conv_mfma"
    assert small["dres2.0.blocks.0"] == "conv_mfma" and small["e1.0"] == "conv_mfma"


def test_frontalizer_from_reference_checkpoints(tmp_path):
    """from_checkpoints on a directory in the reference's layout (ngf = 4): flowNetF bit-equal to the reference-written file, and the
    composed forward (torch backend) against the reference's test_forward fixture."""
    import test_trainer_cpu as T
    import ffwm_amd
    torch.set_num_threads(8)
    gold, ckpt_dir = T._eval_golden()
    ep = T._prepare_reference_checkpoints(tmp_path, gold, ckpt_dir)
    f = ffwm_amd.Frontalizer.from_checkpoints(str(tmp_path), ep, ngf=4, device="cpu", graph=False, backend="torch")
    ref_sd = torch.load(os.path.join(ckpt_dir, "%s_net_flowNetF.pth" % ep))
    sd = f.flow.state_dict()
    assert list(sd) == list(ref_sd)
    for k, v in sd.items():
        assert torch.equal(v, ref_sd[k]), k
    r = f(fill.image(2, 3, 128, 128, "eval_img_S"))
    tf = gold["test_forward"]
    for got, key in zip(r.flows, ("flow_F128", "flow_F64", "flow_F32")):
        T._packed_close(got, tf[key], 1e-5)
    T._packed_close(r.img_S_warp, tf["img_S_warp"], 1e-5)
    T._packed_close(r.fake_F128, tf["fake_F128"], 1e-4)
    T._packed_close(r.att, tf["att"], 1e-4)
    assert r.fake_F64.shape == (2, 3, 64, 64) and r.fake_F32.shape == (2, 3, 32, 32)
    with pytest.raises(ValueError):
        ffwm_amd.Frontalizer.from_checkpoints(str(tmp_path), ep, ngf=4, device="cpu", graph=True, backend="torch")


# ---------------------------------------------------------------------------------------------- the C ABI of csrc/netg_eval.hip
@pytest.fixture(scope="module")
def hiplib():
    from ffwm_amd import build, _lib
    build.build()
    return _lib.load()


NEW_SYMBOLS = ["ffwm_shuffle_bias_act_forward", "ffwm_image_head_forward", "ffwm_upsample2x_bilinear_forward",
               "ffwm_sigmoid_gate_forward_strided"]


def test_new_symbols_are_exported_and_bound(hiplib):
    from ffwm_amd import _lib
    for n in NEW_SYMBOLS:
        assert hasattr(hiplib, n) and n in _lib.EXPORTS
    assert hiplib.ffwm_abi_version() == 5


def test_netg_eval_argument_errors_are_reported_before_launch(hiplib):
    """NULL pointer -> FFWM_ERR_ARG (-1), float64 -> FFWM_ERR_DTYPE (-2), a zero size -> -1, a batch stride smaller than one sample
    of the destination view -> -1; nothing touches a device."""
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    F32, F64 = 0, 1
    err = hiplib.ffwm_last_error

    def shuffle(h=p, y=p, K=2, H=4, stride=2 * 4 * 16, dt=F32):
        return hiplib.ffwm_shuffle_bias_act_forward(h, p, y, 1, K, H, 4, stride, 0.2, dt, None)

    def head(x=p, w=p, y=p, C=5, H=4, stride=3 * 16, dt=F32):
        return hiplib.ffwm_image_head_forward(x, w, p, y, 1, C, H, 4, stride, dt, None)

    def up(x=p, y=p, C=3, H=4, stride=3 * 4 * 16, dt=F32):
        return hiplib.ffwm_upsample2x_bilinear_forward(x, y, 1, C, H, 4, stride, dt, None)

    def gate(a=p, x=p, y=p, C=3, HW=16, stride=3 * 16, dt=F32):
        return hiplib.ffwm_sigmoid_gate_forward_strided(a, p, x, None, y, 1, C, HW, stride, dt, None)

    assert shuffle(h=None) == -1 and b"NULL" in err()
    assert shuffle(y=None) == -1 and b"NULL" in err()
    assert shuffle(dt=F64) == -2 and b"float32" in err()
    assert shuffle(K=0) == -1 and shuffle(H=0) == -1
    assert shuffle(stride=2 * 4 * 16 - 1) == -1 and b"batch stride" in err()

    assert head(x=None) == -1 and b"NULL" in err()
    assert head(w=None) == -1 and head(y=None) == -1
    assert head(dt=F64) == -2 and b"float32" in err()
    assert head(C=0) == -1 and head(H=0) == -1
    assert head(stride=3 * 16 - 1) == -1 and b"batch stride" in err()

    assert up(x=None) == -1 and b"NULL" in err()
    assert up(y=None) == -1
    assert up(dt=F64) == -2 and b"float32" in err()
    assert up(C=0) == -1 and up(H=0) == -1
    assert up(stride=3 * 4 * 16 - 1) == -1 and b"batch stride" in err()

    assert gate(a=None) == -1 and b"NULL" in err()
    assert gate(x=None) == -1 and gate(y=None) == -1
    assert gate(dt=F64) == -2 and b"float32" in err()
    assert gate(C=0) == -1 and gate(HW=0) == -1
    assert gate(stride=3 * 16 - 1) == -1 and b"batch stride" in err()
    # planes past the index range of the kernels
    assert hiplib.ffwm_upsample2x_bilinear_forward(p, p, 1, 1, 1 << 14, 4, 1 << 40, F32, None) == -3
    assert hiplib.ffwm_shuffle_bias_act_forward(p, p, p, 1, 1, 1 << 15, 4, 1 << 40, 0.2, F32, None) == -3


def test_ops_wrappers_refuse_cpu_tensors():
    from ffwm_amd import ops
    x = torch.zeros(1, 4, 4, 4)
    with pytest.raises(NotImplementedError):
        ops.shuffle_bias_act(x, torch.zeros(1))
    with pytest.raises(NotImplementedError):
        ops.image_head(x, torch.zeros(3, 4, 3, 3), torch.zeros(3))
    with pytest.raises(NotImplementedError):
        ops.upsample2x_bilinear(x)
    with pytest.raises(NotImplementedError):
        ops.sigmoid_gate_forward_strided(x, x, x)

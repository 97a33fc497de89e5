"""csrc/netg_eval.hip, FoldedFFWM and Frontalizer (ffwm_amd/ffwm_eval.py) on the MI355X -- run with ``-m gpu``.

Guard convention: every destination-view test writes into a channel slice of a wider buffer pre-filled with NaN (so the batch stride
is larger than the slice) and asserts that the channels outside the slice still hold NaN afterwards.

Every netG carries the closed-form weights of tests/golden/fill.py (a default-initialised FFWM(sn=True) overflows in eval mode)."""
import copy
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import fill  # noqa: E402
import torch_refs  # noqa: E402

DEV = "cuda:0"
EPS32 = float(torch.finfo(torch.float32).eps)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _guarded(B, C, H, W, before=2, after=3):
    """(buffer of NaN [B, before + C + after, H, W], its channel slice [before : before + C], check()): check asserts that the guard
    channels still hold NaN and that the slice holds none."""
    buf = torch.full((B, before + C + after, H, W), float("nan"), device=DEV)
    view = buf[:, before:before + C]

    def check():
        assert torch.isnan(buf[:, :before]).all() and torch.isnan(buf[:, before + C:]).all(), "a write outside the destination view"
        assert not torch.isnan(view).any(), "the destination view was not fully written"
    return buf, view, check


# ---------------------------------------------------------------------------------------------------- the four kernels
# the last two pass one sweep of the 2048-block grid (524 288 threads) on the vector and on the scalar route: h is [1, 132, 256, 256]
# and [1, 36, 241, 243]
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 64, 16, 16), (1, 33, 256, 256), (1, 9, 241, 243)])
def test_shuffle_bias_act(shape):
    """One add and one multiply per element, nothing to reassociate: equal to the PyTorch composition bit for bit."""
    from ffwm_amd import ops
    B, K, H, W = shape
    h = torch.randn(B, 4 * K, H, W, generator=_gen(1)).to(DEV)
    bias = torch.randn(K, generator=_gen(2)).to(DEV)
    assert (h + bias.repeat_interleave(4).view(1, -1, 1, 1) > 0).any() and (h + bias.repeat_interleave(4).view(1, -1, 1, 1) < 0).any()
    ref = F.leaky_relu(F.pixel_shuffle(h, 2) + bias.view(1, -1, 1, 1), 0.2)
    _, view, check = _guarded(B, K, 2 * H, 2 * W)
    assert view.stride(0) > K * 4 * H * W
    out = ops.shuffle_bias_act(h, bias, 0.2, out=view)
    check()
    assert torch.equal(out, ref)
    assert torch.equal(ops.shuffle_bias_act(h, bias, 0.2), ref)          # a fresh contiguous destination


# (the last two: past 524 288 threads, four output pixels per lane and one)
@pytest.mark.parametrize("shape", [(2, 3, 1, 1), (1, 3, 5, 7), (2, 3, 32, 32), (1, 3, 512, 360), (1, 3, 211, 209)])
def test_upsample2x_bilinear(shape):
    """A four-term combination whose weights and weight products (0.25, 0.75, 0.0625, 0.1875, 0.5625) are exact:
    <= 4 eps32 max|x| against float64 F.interpolate."""
    from ffwm_amd import ops
    B, C, H, W = shape
    x = torch.randn(B, C, H, W, generator=_gen(3)).to(DEV)
    ref = F.interpolate(x.double(), scale_factor=2, mode="bilinear")
    _, view, check = _guarded(B, C, 2 * H, 2 * W)
    out = ops.upsample2x_bilinear(x, out=view)
    check()
    d = (out.double() - ref).abs().max().item()
    bound = 4 * EPS32 * x.abs().max().item()
    print("upsample2x %s: max abs diff %.3e, bound %.3e" % (shape, d, bound))
    assert d <= bound, (d, bound)


# the heads' own shapes and ragged planes (one pixel per lane), then two that reach the four-pixels-per-lane tile (a workgroup for every CU): ragged rows with scalar
# stores, and W % 4 == 0 with 16-byte stores
@pytest.mark.parametrize("shape", [(2, 5, 7, 9), (1, 195, 16, 12), (1, 384, 8, 8), (1, 195, 33, 130), (1, 6, 130, 515), (4, 5, 128, 128)])
def test_image_head(shape):
    """Against float64 sigmoid(conv2d + b): <= 2e-6 max(1, sqrt(9 C) / 4) max|z|, z the float64 pre-activation -- the formula of the
    thin direct convolution (tests/conv_bounds.py); sigmoid's slope is at most 1/4, so the bound carries over to the output."""
    from ffwm_amd import ops
    B, C, H, W = shape
    x = torch.randn(B, C, H, W, generator=_gen(4)).to(DEV)
    w = (torch.randn(3, C, 3, 3, generator=_gen(5)) / (9 * C) ** 0.5).to(DEV)
    b = (0.1 * torch.randn(3, generator=_gen(6))).to(DEV)
    z = F.conv2d(x.double(), w.double(), b.double(), 1, 1)
    ref = torch.sigmoid(z)
    _, view, check = _guarded(B, 3, H, W, before=1, after=1)
    out = ops.image_head(x, w, b, out=view)
    check()
    d = (out.double() - ref).abs().max().item()
    bound = 2e-6 * max(1.0, (9 * C) ** 0.5 / 4) * z.abs().max().item()
    print("image_head %s: max abs diff %.3e, bound %.3e" % (shape, d, bound))
    assert d <= bound, (d, bound)
    assert torch.equal(ops.image_head(x, w, b), out)                      # a contiguous destination; partial sums meet in a fixed order


@pytest.mark.parametrize("want_att", [True, False])
@pytest.mark.parametrize("shape", [(2, 6, 5, 7), (1, 256, 8, 8)])
def test_sigmoid_gate_forward_strided(shape, want_att):
    from ffwm_amd import ops
    a, b, x = (torch.randn(*shape, generator=_gen(s)).to(DEV) for s in (7, 8, 9))
    y_ref, att_ref = ops.sigmoid_gate_forward(a, b, x)
    B, C, H, W = shape
    _, view, check = _guarded(B, C, H, W)
    y, att = ops.sigmoid_gate_forward_strided(a, b, x, out=view, want_att=want_att)
    check()
    assert torch.equal(y, y_ref)
    assert (att is None) if not want_att else torch.equal(att, att_ref)


# ---------------------------------------------------------------------------------------------------- FoldedFFWM
FEATURES = ["e0", "e1", "e2", "e3", "d0", "d1", "d2", "dres0", "dres1", "dres2"]


@pytest.fixture(scope="module")
def filled():
    """The filled full-width netG on the GPU (torch warps: the float64 reference copies are made from it) and its folded form."""
    from ffwm_amd import nets
    from ffwm_amd.ffwm_eval import FoldedFFWM
    net = fill.fill_module(nets.FFWM(sn=True, warp_flipcat=torch_refs.warp_flipcat)).to(DEV).eval()
    return net, FoldedFFWM(net, graph=False), copy.deepcopy(net).double()


def _module_features(net, img, flows):
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


@pytest.mark.parametrize("shape", [(2, 32, 32), (1, 48, 40)])
def test_folded_ffwm_full_width_against_float64(filled, shape):
    """Outputs and every return_features tensor against the float64 module on the GPU: <= 1e-4 max|ref| per tensor."""
    net, folded, net64 = filled
    B, H, W = shape
    img = fill.image(B, 3, H, W, "netG_in").to(DEV)
    flows = [fill.flow_field(B, H // s, W // s, "netG_flow%d" % (H // s)).to(DEV) for s in (4, 2, 1)]
    r32, r64, r128, att, feats = folded(img, flows, return_att=True, return_features=True)
    assert folded.last_launches == folded.plan(B, H, W)
    ref_out, ref_feats = _module_features(net64, img.double(), [f.double() for f in flows])
    pairs = [(n, feats[n], ref_feats[n]) for n in FEATURES] + list(zip(("rec32", "rec64", "rec128", "att"), (r32, r64, r128, att), ref_out))
    bad = []
    for name, got, ref in pairs:
        assert got.shape == ref.shape, name
        rel = (got.double() - ref).abs().max().item() / ref.abs().max().item()
        print("folded %s %-6s rel %.3e" % (shape, name, rel))
        if not rel <= 1e-4:
            bad.append((name, rel))
    assert not bad, bad
    r = folded(img, flows)                                       # without the attention map: three outputs, the same values
    assert len(r) == 3 and torch.equal(r[2], r128)


def test_folded_ffwm_matches_the_reference_fixture(filled):
    gold = torch.load(os.path.join(HERE, "golden", "reference_modules.pt"))["ffwm_eval"]
    _, folded, _ = filled
    img = fill.image(1, 3, 128, 128, "netG_in").to(DEV)
    flows = [fill.flow_field(1, s, s, "netG_flow%d" % s).to(DEV) for s in (32, 64, 128)]
    r32, r64, r128, att = folded(img, flows, return_att=True)
    kinds = set(k for _, k in folded.last_launches)
    assert "winograd" in kinds and "conv_mfma" in kinds          # the large planes reach the Winograd kernel at this size
    for name, got, ref in (("rec32", r32, gold["rec32"]), ("rec64", r64, gold["rec64"]), ("rec128", r128[..., ::2, ::2], gold["rec128_s2"]),
                           ("att", att[..., ::8, ::8], gold["att_s8"])):
        d = (got.cpu() - ref).abs().max().item()
        print("fixture %s: max abs diff %.3e" % (name, d))
        assert d <= 1e-4, (name, d)
    assert abs(r128.double().sum().item() - gold["sum128"].item()) < 0.2
    assert abs(att.double().sum().item() - gold["att_sum"].item()) < 2.0


def test_folded_ffwm_graph_replay(filled):
    """graph=True: the replayed forward follows its inputs and agrees with the eager one to the fp32 contract (not bit for bit: the
    Winograd kernel's four-way reduction split meets in float atomics)."""
    from ffwm_amd.ffwm_eval import FoldedFFWM
    net, eager, _ = filled
    g = FoldedFFWM(net, graph=True)
    for tag in ("netG_in", "eval_img_S"):
        img = fill.image(1, 3, 128, 128, tag).to(DEV)
        flows = [fill.flow_field(1, s, s, "%s_flow%d" % (tag, s)).to(DEV) for s in (32, 64, 128)]
        got = [t.clone() for t in g(img, flows, return_att=True)]
        ref = eager(img, flows, return_att=True)
        for a, b in zip(got, ref):
            assert (a - b).abs().max().item() <= 1e-4 * b.abs().max().item()
    assert g._graph is not None


def test_spectral_norm_snapshot_of_a_fused_network(filled):
    """A net that went through fuse_spectral_norm: the snapshot equals the weights its batched kernel sets in an eval forward
    within 2 eps32 max|w|."""
    from ffwm_amd.spectral_norm import fuse_spectral_norm
    net, folded, _ = filled
    fused = copy.deepcopy(net)
    fuse_spectral_norm(fused)
    img = fill.image(1, 3, 32, 32, "netG_in").to(DEV)
    flows = [fill.flow_field(1, s, s, "netG_flow%d" % s).to(DEV) for s in (8, 16, 32)]
    with torch.no_grad():
        fused(img, flow=flows)
    assert len(folded.sn_weights) == 52
    for p, w_snap in folded.sn_weights.items():
        w = fused.get_submodule(p).weight
        d = (w_snap - w).abs().max().item()
        assert d <= 2 * EPS32 * w.abs().max().item(), (p, d)


# ---------------------------------------------------------------------------------------------------- Frontalizer
def _close(got, ref, tol):
    d = (got - ref).abs().max().item()
    assert d <= tol * (1.0 + ref.abs().max().item()), (d, tol)
    return d


@pytest.fixture(scope="module")
def frontalizers(tmp_path_factory):
    """Frontalizer.from_checkpoints on a checkpoint directory in the reference's layout (ngf = 4): captured and eager."""
    import test_trainer_cpu as T
    import ffwm_amd
    gold, ckpt_dir = T._eval_golden()
    d = tmp_path_factory.mktemp("ckpt")
    ep = T._prepare_reference_checkpoints(d, gold, ckpt_dir)
    captured = ffwm_amd.Frontalizer.from_checkpoints(str(d), ep, ngf=4, device=DEV, graph=True)
    eager = ffwm_amd.Frontalizer.from_checkpoints(str(d), ep, ngf=4, device=DEV, graph=False)
    return T, gold, captured, eager


def test_frontalizer_matches_the_reference_composed_forward(frontalizers):
    T, gold, f, _ = frontalizers
    r = f(fill.image(2, 3, 128, 128, "eval_img_S").to(DEV))
    tf = gold["test_forward"]
    for got, key in zip(r.flows, ("flow_F128", "flow_F64", "flow_F32")):
        print(key, T._packed_close(got, tf[key], 1e-4))
    print("img_S_warp", T._packed_close(r.img_S_warp, tf["img_S_warp"], 1e-4))
    print("fake_F128", T._packed_close(r.fake_F128, tf["fake_F128"], 1e-4))
    print("att", T._packed_close(r.att, tf["att"], 1e-4))
    assert r.fake_F64.shape == (2, 3, 64, 64) and r.fake_F32.shape == (2, 3, 32, 32) and r.att.shape == (2, 1, 128, 128)


def test_frontalizer_graph_replay_follows_its_input(frontalizers):
    """A second call with another image: the static outputs change, and agree with an eager Frontalizer on that image to the same
    bound (not bit for bit: the Winograd kernel's four-way reduction split meets in float atomics)."""
    _, _, f, eager = frontalizers
    first = f(fill.image(2, 3, 128, 128, "eval_img_S").to(DEV))
    first = [first.fake_F128.clone(), first.img_S_warp.clone(), first.att.clone(), first.flows[0].clone()]
    img = fill.image(2, 3, 128, 128, "eval_img_F").to(DEV)
    r = f(img)
    assert f._graph is not None
    second = [r.fake_F128, r.img_S_warp, r.att, r.flows[0]]
    for a, b in zip(first, second):
        assert not torch.equal(a, b)
    e = eager(img)
    for name in ("fake_F128", "fake_F64", "fake_F32", "img_S_warp", "att"):
        print(name, _close(getattr(r, name), getattr(e, name), 1e-4))
    for a, b in zip(r.flows, e.flows):
        _close(a, b, 1e-4)

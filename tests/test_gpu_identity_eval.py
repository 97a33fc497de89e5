"""csrc/lightcnn_eval.hip, FoldedLightCNN and FaceIdentifier (ffwm_amd/identity_eval.py) on the MI355X -- run with ``-m gpu``.
Bounds and input families: tests/identity_bounds.py."""
import copy
import itertools
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
import identity_bounds as ib  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")


def _dev(t):
    return None if t is None else t.to(DEV)


# ---------------------------------------------------------------------------------------------------- mfm_tail
@pytest.mark.parametrize("with_bias,with_res,pool", list(itertools.product([False, True], repeat=3)))
@pytest.mark.parametrize("shape", ib.TAIL_SHAPES)
def test_mfm_tail_equals_the_torch_composition(shape, with_bias, with_res, pool):
    """Bit for bit (same NaN positions), into a batch slice of a NaN-guarded wider buffer; NaN planted in the windows that hang
    over the edge travels as in ATen."""
    from ffwm_amd import ops
    B, C2, H, W = shape
    C = C2 // 2
    route, items, past = ib.tail_route(shape, pool)
    assert route == ("vector" if W % 4 == 0 else "scalar")
    if H >= 400:
        assert past, "the two large shapes pass one sweep of the grid on every combination"
    h, bias, res = ib.tail_inputs(shape, 11 + B + H, with_bias, with_res, pool)
    ref = ib.tail_reference(h, bias, res, pool)
    Ho, Wo = ref.shape[2:]
    assert (Ho, Wo) == (((H + 1) // 2, (W + 1) // 2) if pool else (H, W))
    assert torch.isnan(ref).any() and (ref.numel() <= 4 or not torch.isnan(ref).all())
    buf = torch.full((2 + B + 1, C, Ho, Wo), NAN, device=DEV)
    view = buf[2:2 + B]
    out = ops.mfm_tail(_dev(h), _dev(bias), _dev(res), pool, out=view)
    assert out.data_ptr() == view.data_ptr()
    assert torch.isnan(buf[:2]).all() and torch.isnan(buf[2 + B:]).all(), "a write outside the destination"
    ib.assert_same(out, ref, "mfm_tail %s bias %s residual %s pool %s" % (shape, with_bias, with_res, pool))
    ib.assert_same(ops.mfm_tail(_dev(h), _dev(bias), _dev(res), pool), ref, "fresh destination")


def test_mfm_tail_refuses_what_it_does_not_serve():
    from ffwm_amd import ops
    h = torch.zeros(1, 4, 3, 3, device=DEV)
    with pytest.raises(NotImplementedError):
        ops.mfm_tail(h.cpu(), None)
    with pytest.raises(NotImplementedError):
        ops.mfm_tail(h.double(), None)
    with pytest.raises(ValueError):
        ops.mfm_tail(h[:, :3], None)
    with pytest.raises(ValueError):
        ops.mfm_tail(h, None, residual=torch.zeros(1, 2, 3, 2, device=DEV))
    with pytest.raises(ValueError):
        ops.mfm_tail(h, None, pool=True, out=torch.zeros(1, 2, 3, 3, device=DEV))


# ---------------------------------------------------------------------------------------------------- identity_input
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 1, 128, 128), (3, 3, 128, 128)])
def test_identity_input_gray(shape):
    from ffwm_amd import ops
    img = torch.randn(shape, generator=torch.Generator().manual_seed(3))
    ref, bound = ib.gray_bound(img)
    out = ops.identity_input(img.to(DEV))
    assert out.shape == (shape[0], 1) + shape[2:]
    r = ib.worst_ratio(out, ref, bound + 1e-45)
    print("identity_input gray %s: error / bound %.3g" % (shape, r))
    assert r <= 1.0
    if shape[1] == 1:
        assert torch.equal(out.cpu(), img)


@pytest.mark.parametrize("case", ["fixture", "one_channel", "three"])
def test_identity_input_crop(case):
    """Per element against the float64 composition from the float64 grid formula, within the bound ATen's own fp32 composition is
    shown to meet on the CPU; the reference's fixture tensor lies inside it too."""
    from ffwm_amd import ops
    gen = torch.Generator().manual_seed(5)
    img = {"fixture": lambda: fill.image(2, 3, 128, 128, "ident_img"), "one_channel": lambda: torch.rand(1, 1, 128, 128, generator=gen),
           "three": lambda: torch.randn(3, 3, 128, 128, generator=gen)}[case]()
    ref, bound = ib.crop_bound(img)
    out = ops.identity_input(img.to(DEV), crop=True)
    assert out.shape == (img.shape[0], 1, 128, 128)
    r = ib.worst_ratio(out, ref, bound)
    print("identity_input crop %s: error / bound %.3g" % (case, r))
    assert r <= 1.0
    if case == "fixture":
        gold = torch.load(os.path.join(HERE, "golden", "reference_identity.pt"))
        assert ib.worst_ratio(gold["cropped"], ref, bound) <= 1.0
        aten = F.interpolate(F.grid_sample(img.to(DEV).mean(1, keepdim=True), _crop_grid(img.shape[0]).permute(0, 2, 3, 1), mode="bilinear",
                                           padding_mode="zeros", align_corners=False), (128, 128), mode="bilinear")
        print("   ATen on the device: error / bound %.3g" % ib.worst_ratio(aten, ref, bound))
    with pytest.raises(ValueError):
        ops.identity_input(torch.zeros(1, 3, 64, 64, device=DEV), crop=True)


def _crop_grid(b):
    from ffwm_amd.identity_eval import crop_grid
    return crop_grid(b, device=DEV)


# ---------------------------------------------------------------------------------------------------- cosine_topk
# the last two need more than one selection block per probe row (2048 gallery rows per block): 3 segments and a merge; the last one
# with rows of 1024 floats, the widest the kernel takes
@pytest.mark.parametrize("dims", [(1, 10, 256, 10), (3, 37, 256, 10), (8, 250, 256, 10), (2, 1000, 7, 32), (9, 5000, 64, 10), (2, 4100, 1024, 32)])
def test_cosine_topk(dims):
    from ffwm_amd import ops
    B, G, D, k = dims
    probe, gallery = ib.separated_gallery(B, G, D, 17)
    ref, bound = ib.cosine_reference(probe, gallery)
    assert ib.rank_gaps(ref, k) > ib.RANK_GAP                    # a condition on the inputs
    assert ib.rank_gaps(ref, k) > 2 * float(bound.max())         # ... under which the fp32 ranks ARE the float64 ranks
    want_val, want_idx = torch.topk(ref, k, dim=1)
    val, idx = ops.cosine_topk(probe.to(DEV), gallery.to(DEV), k)
    assert val.shape == (B, k) and idx.shape == (B, k) and idx.dtype == torch.int32 and val.dtype == torch.float32
    assert torch.equal(idx.cpu().long(), want_idx)
    r = ib.worst_ratio(val, want_val, torch.gather(bound, 1, want_idx))
    print("cosine_topk %s: value error / bound %.3g" % (dims, r))
    assert r <= 1.0
    val2, idx2 = ops.cosine_topk(probe.to(DEV), gallery.to(DEV), k)
    assert torch.equal(val, val2) and torch.equal(idx, idx2)      # deterministic


@pytest.mark.parametrize("G", [40, 4500])
def test_cosine_topk_ties_zero_rows_and_nan(G):
    """Duplicated gallery rows: equal similarity, the lower index first (across selection blocks too); a zero row: the eps clamp gives
    similarity 0, not NaN; a NaN row ranks above everything."""
    from ffwm_amd import ops
    B, D, k = 3, 64, 12
    probe, gallery = ib.separated_gallery(B, G, D, 23)
    ref0, _ = ib.cosine_reference(probe, gallery)
    lead = torch.topk(ref0, 2, dim=1)[1]                          # each probe's two leaders
    dup = [3, G // 2, G - 2]                                      # copies of probe 0's leader, scattered
    for j in dup:
        gallery[j] = gallery[lead[0, 0]]
    taken = set(dup) | set(lead.flatten().tolist())
    zero = next(j for j in range(5, 32) if j not in taken)
    nan_row = next(j for j in range(G - 5, 0, -1) if j not in taken)
    gallery[zero] = 0.0
    ref, bound = ib.cosine_reference(probe, gallery)
    val, idx = ops.cosine_topk(probe.to(DEV), gallery.to(DEV), k)
    val, idx = val.cpu(), idx.cpu().long()
    tied = sorted(set(dup + [int(lead[0, 0])]))
    n = len(tied)
    assert n >= 3 and idx[0, :n].tolist() == tied and torch.equal(val[0, :n], val[0, :1].expand(n))
    assert torch.all(val[:, :-1] >= val[:, 1:])
    assert ib.worst_ratio(val, torch.gather(ref, 1, idx), torch.gather(bound, 1, idx)) <= 1.0
    # the zero row: similarity exactly 0 for every probe
    full_val, full_idx = ops.cosine_topk(probe.to(DEV), gallery[:32].contiguous().to(DEV), 32)
    pos = (full_idx.cpu() == zero).nonzero()
    assert pos.shape[0] == B and torch.all(full_val.cpu()[pos[:, 0], pos[:, 1]] == 0.0)
    # a zero probe row as well
    zp = probe.clone()
    zp[1] = 0.0
    zval, _ = ops.cosine_topk(zp.to(DEV), gallery.to(DEV), k)
    assert torch.all(zval.cpu()[1] == 0.0) and not torch.isnan(zval).any()
    # NaN: above everything, for every probe
    gallery[nan_row, 3] = NAN
    nval, nidx = ops.cosine_topk(probe.to(DEV), gallery.to(DEV), k)
    assert torch.all(nidx.cpu()[:, 0] == nan_row) and torch.isnan(nval.cpu()[:, 0]).all() and not torch.isnan(nval.cpu()[:, 1:]).any()
    assert nidx.cpu()[0, 1:1 + n].tolist() == tied


def test_cosine_topk_refuses_what_it_does_not_serve():
    from ffwm_amd import ops
    p, g = torch.zeros(2, 8, device=DEV), torch.zeros(5, 8, device=DEV)
    for bad in (lambda: ops.cosine_topk(p, g, 6), lambda: ops.cosine_topk(p, g, 0), lambda: ops.cosine_topk(p, g[:, :7].contiguous(), 1),
                lambda: ops.cosine_topk(torch.zeros(2, 1025, device=DEV), torch.zeros(5, 1025, device=DEV), 1)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(NotImplementedError):
        ops.cosine_topk(p.cpu(), g, 1)


# ---------------------------------------------------------------------------------------------------- FoldedLightCNN
@pytest.fixture(scope="module")
def seeded():
    """The well-conditioned, input-following LightCNN-29 of tests/identity_bounds.py on the device, its folded form and its float64
    copy."""
    from ffwm_amd.identity_eval import FoldedLightCNN
    net = ib.conditioned_lightcnn().to(DEV)
    return net, FoldedLightCNN(net), copy.deepcopy(net).double()


@pytest.mark.parametrize("shape", [(2, 128, 128), (1, 120, 120)])
def test_folded_lightcnn_against_float64(seeded, shape):
    """fc and pool against the float64 module: <= 1e-4 max|ref| per tensor, FoldedFFWM's contract."""
    net, folded, net64 = seeded
    B, H, W = shape
    x = fill.image(B, 1, H, W, "lightcnn_in").to(DEV)
    fc, pool = folded(x)
    assert folded.backend == "hip" and folded.last_launches == folded.plan(B, H, W)
    with torch.no_grad():
        _, fc64, pool64 = net64(x.double())
    assert fc.shape == fc64.shape == (B, 256) and pool.shape == pool64.shape == (B, 128, 8, 8)
    for name, got, ref in (("fc", fc, fc64), ("pool", pool, pool64)):
        rel = (got.double() - ref).abs().max().item() / ref.abs().max().item()
        print("folded lightcnn %s %-4s rel %.3e" % (shape, name, rel))
        assert rel <= 1e-4, (name, rel)
    kinds = [k for _, k in folded.last_launches]
    assert kinds.count("mfm_tail") == 29
    # the network follows its input: a structured image moves fc by most of its size (a condition on the network and the inputs),
    # and the folded path is held to the same bound there
    xs = ib.structured_image(B, H, W).to(DEV)
    with torch.no_grad():
        _, other, _ = net64(xs.double())
    moved = (other - fc64).abs().max().item() / fc64.abs().max().item()
    rel = (folded(xs)[0].double() - other).abs().max().item() / other.abs().max().item()
    print("   a structured image moves fc by %.3e of max|fc|; folded against float64 on it: rel %.3e" % (moved, rel))
    assert moved >= 0.1 and rel <= 1e-4


def test_folded_lightcnn_against_the_reference_fixture():
    """The filled network of the reference's fixture is ill-conditioned: fp32 rounding alone moves its outputs by percent.  RMS bounds
    from the reference's own distance to float64 (tests/identity_bounds.py), taken on BOTH machines: the fixture's (the CPU that made
    it) and that of nets.LightCNN29 -- the module path, the vendor's convolutions -- on this device.  Measured on the MI355X, rms
    error of fc at batch 2: fixture 1.09e-3, module path on the device 6.23e-3, FoldedLightCNN 6.27e-3 (with every layer on the
    vendor's convolution: 6.23e-3, the module path's own figure); rms(fc) = 0.127.  The CPU figure alone does not describe the
    device: the module path misses 4 x 1.09e-3 exactly as the folded path does."""
    from ffwm_amd import nets
    from ffwm_amd.identity_eval import FoldedLightCNN
    g = torch.load(os.path.join(HERE, "golden", "reference_modules.pt"))["lightcnn_eval"]
    net = fill.fill_module(nets.LightCNN29()).eval()
    x = fill.image(2, 1, 128, 128, "lightcnn_in")
    with torch.no_grad():
        _, fc64, pool64 = copy.deepcopy(net).double()(x.double())          # on the CPU, as the fixture was made
        net = net.to(DEV)
        _, fc_mod, pool_mod = net(x.to(DEV))                                # the module path on this device
    fc, pool = FoldedLightCNN(net)(x.to(DEV))

    def rms(t):
        return t.double().pow(2).mean().sqrt().item()
    for name, got, mod, fix, ref in (("fc", fc.cpu(), fc_mod.cpu(), g["fc"], fc64),
                                     ("pool", pool.cpu()[..., ::2, ::2], pool_mod.cpu()[..., ::2, ::2], g["pool_s2"], pool64[..., ::2, ::2])):
        e_cpu, e_dev = rms(fix - ref), rms(mod - ref)
        e_ref = max(e_cpu, e_dev)
        e64, efix = rms(got - ref), rms(got - fix)
        print("fixture %-4s: rms(ref) %.3e, reference's error: fixture %.3e, module on the device %.3e; rms(got - float64) %.3e, "
              "rms(got - fixture) %.3e" % (name, rms(ref), e_cpu, e_dev, e64, efix))
        assert e_ref <= 0.1 * rms(ref)
        assert e64 <= ib.SAFETY * e_ref and efix <= (ib.SAFETY + 1) * e_ref, (name, e_ref, e64, efix)


def test_folded_lightcnn_graph_replay_follows_its_input(seeded):
    from ffwm_amd.identity_eval import FoldedLightCNN
    net, eager, _ = seeded
    g = FoldedLightCNN(net, graph=True)
    outs = []
    for x in (fill.image(2, 1, 128, 128, "lightcnn_in").to(DEV), ib.structured_image(2, 128, 128).to(DEV)):
        got = [t.clone() for t in g(x)]
        ref = eager(x)
        for a, b in zip(got, ref):
            assert (a - b).abs().max().item() <= 1e-4 * b.abs().max().item()
        outs.append(got)
    moved = (outs[0][0] - outs[1][0]).abs().max().item()
    assert g._graph is not None and moved >= 0.1 * outs[0][0].abs().max().item()          # far above the 1e-4 it is held to
    with pytest.raises(ValueError):
        FoldedLightCNN(net, graph=True, backend="torch")


# ---------------------------------------------------------------------------------------------------- FaceIdentifier
def _close(got, ref, tol):
    d = (got - ref).abs().max().item()
    assert d <= tol * (1.0 + ref.abs().max().item()), (d, tol)
    return d


@pytest.fixture(scope="module")
def identifiers(tmp_path_factory):
    """FaceIdentifier.from_checkpoints on a checkpoint directory in the reference's layout (ngf = 4) and a filled LightCNN saved as a
    plain state dict: captured and eager, with the gallery of tests/identity_bounds.py."""
    import test_trainer_cpu as T
    import ffwm_amd
    gold, ckpt_dir = T._eval_golden()
    d = tmp_path_factory.mktemp("ident")
    ep = T._prepare_reference_checkpoints(d, gold, ckpt_dir)
    light = ib.saved_lightcnn(os.path.join(str(d), "lightcnn.pth"))
    captured = ffwm_amd.FaceIdentifier.from_checkpoints(str(d), ep, light, ngf=4, device=DEV, graph=True)
    eager = ffwm_amd.FaceIdentifier.from_checkpoints(str(d), ep, light, ngf=4, device=DEV, graph=False)
    cropped = ffwm_amd.FaceIdentifier.from_checkpoints(str(d), ep, light, ngf=4, crop=True, device=DEV, graph=False)
    # the same with the well-conditioned network of tests/identity_bounds.py, for comparisons across arithmetics
    net = ib.conditioned_lightcnn()
    plain = os.path.join(str(d), "lightcnn_seeded.pth")
    torch.save(net.state_dict(), plain)
    cropped_plain = ffwm_amd.FaceIdentifier.from_checkpoints(str(d), ep, plain, ngf=4, crop=True, device=DEV, graph=True)
    return T, gold, captured, eager, (cropped, cropped_plain)


def test_face_identifier_captured_against_eager(identifiers):
    T, gold, f, eager, _ = identifiers
    keys, gallery, probes, probes2 = ib.identifier_case()
    probes, probes2 = probes.to(DEV), probes2.to(DEV)
    r = f(probes[:2])
    assert r.top_sim is None and r.top_idx is None and r.feature.shape == (2, 256)          # before set_gallery
    print("fake_F128", T._packed_close(r.frontal.fake_F128, gold["test_forward"]["fake_F128"], 1e-4))
    for ident in (f, eager):
        ident.set_gallery(keys, gallery.to(DEV))
        assert ident.k == 10
    print("gallery features", _close(f.gallery_features, eager.gallery_features, 1e-4))
    r = f(probes)
    assert f._graph is not None
    first = [r.frontal.fake_F128.clone(), r.feature.clone(), r.top_sim.clone(), r.top_idx.clone()]
    e = eager(probes)
    assert r.top_idx.shape == (4, 10) and r.top_idx.dtype == torch.int32 and r.top_sim.shape == (4, 10)
    print("feature", _close(first[1], e.feature, 1e-4))
    print("top_sim", _close(first[2], e.top_sim, 1e-4))
    ok = ib.qualifying_rows(e.top_sim)
    assert ok.float().mean().item() >= 0.9
    assert torch.equal(first[3].cpu()[ok], e.top_idx.cpu()[ok])
    # the eager matcher is torch's on the eager feature
    sims = torch.stack([torch.cosine_similarity(eager.gallery_features, e.feature[b:b + 1], dim=1) for b in range(4)])
    assert torch.equal(torch.topk(sims.double(), 10, dim=1)[1].cpu()[ok], e.top_idx.cpu().long()[ok])
    # a second call with another image: the static outputs change and follow it
    r2 = f(probes2)
    e2 = eager(probes2)
    assert not torch.equal(first[0], r2.frontal.fake_F128) and not torch.equal(first[1], r2.feature) and not torch.equal(first[2], r2.top_sim)
    print("feature, second call", _close(r2.feature, e2.feature, 1e-4))
    ok2 = ib.qualifying_rows(e2.top_sim)
    assert torch.equal(r2.top_idx.cpu()[ok2], e2.top_idx.cpu()[ok2])
    # eager feature() calls at a batch no capture has seen leave the captured graph's workspaces alone: the replay still holds
    arena_buf = f.net.arena.buf
    for _ in range(3):
        f.feature(torch.cat((gallery, gallery), 0).to(DEV))                # batch 24
    assert f.net.arena.buf is arena_buf
    kept = [r2.feature.clone(), r2.top_sim.clone(), r2.top_idx.clone()]
    junk = [torch.full((1 << 20,), NAN, device=DEV) for _ in range(8)]     # whatever the allocator would hand out again
    r3 = f(probes2)
    _close(r3.feature, kept[0], 1e-4)
    _close(r3.top_sim, kept[1], 1e-4)
    assert torch.equal(r3.top_idx.cpu()[ok2], kept[2].cpu()[ok2])
    del junk
    # the meter takes the indices as they are
    from ffwm_amd import RankMeter
    m = RankMeter()
    m.update(r2.top_idx, ["%s_01_01_050_00.png" % keys[int(i)] for i in e2.top_idx[:, 0]], f.gallery_keys)
    assert m.stat_dict == {"050": {"correct": 4, "all": 4}}


def test_face_identifier_crop_matches_the_reference_steps(identifiers):
    """crop=True against the eager composition of the reference's three steps (mean -> WarpNet(grid98) -> interpolate) on the
    frontalised image.  The network's INPUT is held to the crop's per-element bound.  The FEATURE is compared where a comparison
    across two arithmetics means something: the filled LightCNN of the fixture amplifies a last-bit difference of its input to
    0.1 of a feature of 0.33 (measured), so with it the feature must equal, bit for bit, the same network on the kernel's own output
    (the flag reaches the kernel, gray first, then the crop); with a well-conditioned LightCNN (seeded N(0, 1 / fan_in) weights) the
    feature matches the feature of the eager three steps to 1e-4 (1 + max|ref|): captured, on the frontal image, and through
    feature() on an image with structure, where that tolerance is twenty times below what the crop itself moves (asserted)."""
    from ffwm_amd import ops
    from ffwm_amd.identity_eval import FoldedLightCNN, torch_identity_input
    _, _, _, eager, (cropped, cropped_plain) = identifiers
    _, _, probes, _ = ib.identifier_case()
    probes = probes[:2].to(DEV)
    r = cropped(probes)
    assert r.top_idx is None and r.top_sim is None
    fake = r.frontal.fake_F128
    ref64, bound = ib.crop_bound(fake)
    own = ops.identity_input(fake, crop=True)
    ratio = ib.worst_ratio(own, ref64, bound)
    print("cropped input: error / bound %.3g; against ATen's three steps on the device %.3e"
          % (ratio, (own - torch_identity_input(fake, crop=True)).abs().max().item()))
    assert ratio <= 1.0
    assert torch.equal(r.feature, eager.net(own)[0])
    assert (eager.net(ops.identity_input(fake))[0] - r.feature).abs().max().item() > 1e-3          # the crop is not a no-op
    # a well-conditioned network, captured: the feature of the eager three steps
    rp = cropped_plain(probes)
    assert cropped_plain._graph is not None
    net = FoldedLightCNN(_plain_lightcnn(cropped_plain))
    ref_feature = net(torch_identity_input(rp.frontal.fake_F128, crop=True))[0]
    print("cropped feature (seeded LightCNN), captured against the eager three steps", _close(rp.feature, ref_feature, 1e-4))
    # the frontal image of the filled generator is nearly flat (the crop moves this feature by 1.4e-4 of its size): the same
    # comparison where the crop matters, on get_gallery_fea's path (models/ffwm_model.py:164-176) with an image that has structure
    img = fill.image(2, 3, 128, 128, "ident_img").to(DEV)
    ref_feature = net(torch_identity_input(img, crop=True))[0]
    effect = (net(torch_identity_input(img, crop=False))[0] - ref_feature).abs().max().item()
    print("   feature(): max|ref| %.3e, the crop moves it by %.3e" % (ref_feature.abs().max().item(), effect))
    assert effect > 20 * 1e-4 * (1.0 + ref_feature.abs().max().item())          # a condition on the network and the input
    print("   feature() against the eager three steps", _close(cropped_plain.feature(img), ref_feature, 1e-4))


def _plain_lightcnn(ident):
    """A nets.LightCNN29 that holds the weights an identifier's FoldedLightCNN snapshotted."""
    from ffwm_amd import nets
    net = nets.LightCNN29()
    sd = net.state_dict()
    for name, L in ident.net.layers.items():
        sd[name + ".filter.weight"], sd[name + ".filter.bias"] = L.w, L.b
    sd["fc.filter.weight"], sd["fc.filter.bias"] = ident.net.fc_w, ident.net.fc_b
    net.load_state_dict(sd)
    return net.to(DEV).eval()

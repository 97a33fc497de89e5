"""The split batched-GEMM Winograd route on the GPU (csrc/conv_winograd_gemm_split.hip, ops.conv3x3_wg_split): per-element float64
bounds through both GEMM tiles and the three epilogues, the exact family bit for bit, determinism, the plan rule and the argument
checks, the non-finite contract; and the route through the networks under precision="bf16x3": FoldedLightCNN and FoldedFFWM call by
call against the bound of each layer, the launch counts, graph replay, precision="fp32" as it was; FoldedLightCNN end to end against
float64, FaceIdentifier's top-1 under both precisions.  Cases, bounds and their derivation: wino_split_cases.py."""
import copy
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import conv_bounds as cb  # noqa: E402
import fill  # noqa: E402
import identity_bounds as ib  # noqa: E402
import torch_refs  # noqa: E402
import wino_split_cases as ws  # noqa: E402
from test_gpu_wino_gemm_bounds import _launches, _vs_float64  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

_IDS = dict(ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))


def _three(ops, x, U, b, K, tile=0):
    return {"none": ops.conv3x3_wg_split(x, U, None, "none", K=K, tile=tile),
            "bias": ops.conv3x3_wg_split(x, U, b, "bias", tile=tile),
            "lrelu": ops.conv3x3_wg_split(x, U, b, "lrelu", slope=ws.SLOPE, tile=tile)}


# ---------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("tile", ws.TILES)
@pytest.mark.parametrize("kind", cb.FAMILIES)
@pytest.mark.parametrize("shape", ws.SHAPES, **_IDS)
def test_epilogues_per_element(shape, kind, tile):
    from ffwm_amd import ops
    x, w, b, bounds = ws.split_case(shape, kind)
    U = ops.conv3x3_wg_split_weights(w.cuda())
    for epi, got in _three(ops, x.cuda(), U, b.cuda(), shape[4], tile).items():
        bounds[epi].check(got)


@pytest.mark.parametrize("tile", ws.TILES)
def test_exact_family_bit_for_bit(tile):
    from ffwm_amd import ops
    x, w = ws.split_exact_inputs()
    three, full, hh = ws.split_exact_reference(x, w)
    got = ops.conv3x3_wg_split(x.cuda(), ops.conv3x3_wg_split_weights(w.cuda()), None, "none", K=w.shape[0], tile=tile).cpu()
    assert not torch.equal(three.float(), hh.float()) and not torch.equal(three.float(), full.float())
    bad = (got != three.float()).nonzero()
    assert bad.shape[0] == 0, "%d elements differ from the three-term value, first at %s" % (bad.shape[0], tuple(int(i) for i in bad[0]))


@pytest.mark.parametrize("tile", ws.TILES)
def test_two_calls_agree_bit_for_bit(tile):
    from ffwm_amd import ops
    shape = ws.SHAPES[4]
    x, w, b, _ = ws.split_case(shape, "iid")
    xg, bg = x.cuda(), b.cuda()
    U = ops.conv3x3_wg_split_weights(w.cuda())
    assert torch.equal(U, ops.conv3x3_wg_split_weights(w.cuda()))
    first = _three(ops, xg, U, bg, shape[4], tile)
    for epi, again in _three(ops, xg, U, bg, shape[4], tile).items():
        assert torch.equal(first[epi], again), epi


def test_the_plan_reaches_both_tiles_and_arguments_are_checked():
    """The plan rule of the fp32 route: the 128 x 128 tile exactly when 16 ceil(K / 128) ceil(T / 128) workgroups still cover every
    compute unit, and a call without a fixed tile is the call with that tile."""
    from ffwm_amd import _lib, ops
    lib = _lib.load()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    chosen = set()
    for B, C, H, W, K in ws.SHAPES + [(8, 512, 16, 16, 512), (8, 256, 32, 32, 256), (8, 256, 16, 16, 256), (64, 64, 64, 64, 128)]:
        T = B * ((H + 1) // 2) * ((W + 1) // 2)
        want = 128 if 16 * ((K + 127) // 128) * ((T + 127) // 128) >= cus else 64
        assert ops.conv3x3_wg_split_tile(B, C, H, W, K) == want == ops.conv3x3_wg_tile(B, C, H, W, K), (B, C, H, W, K)
        chosen.add(want)
    assert chosen == {64, 128}
    assert ops.conv3x3_wg_split_tile(0, 8, 4, 4, 8) == 0
    shape = ws.SHAPES[3]
    x, w, b, _ = ws.split_case(shape, "iid")
    xg, bg = x.cuda(), b.cuda()
    U = ops.conv3x3_wg_split_weights(w.cuda())
    assert torch.equal(ops.conv3x3_wg_split(xg, U, bg, "bias"), ops.conv3x3_wg_split(xg, U, bg, "bias", tile=ops.conv3x3_wg_split_tile(*shape)))
    out = torch.empty(1, 64, 32, 32, device=DEV)
    assert ops.conv3x3_wg_split(xg, U, bg, "lrelu", out=out) is out
    p = xg.data_ptr()
    fwd, err = lib.ffwm_conv3x3_wg_split_forward, lib.ffwm_last_error
    assert fwd(None, None, None, None, None, 1, 8, 4, 4, 8, 0, 0.2, 0, 0, None) == -1
    assert fwd(p, p, p, p, p, 1, 8, 4, 4, 8, 3, 0.2, 0, 0, None) == -1 and b"epilogue" in err()
    assert fwd(p, p, p, p, p, 1, 8, 4, 4, 8, 0x100, 0.2, 0, 0, None) == -1          # no hidden bits in the epilogue
    assert fwd(p, p, None, p, p, 1, 8, 4, 4, 8, 2, 0.2, 0, 0, None) == -1 and b"bias" in err()
    assert fwd(p, p, None, p, p, 1, 8, 4, 4, 8, 0, 0.2, 0, 1, None) == -2
    assert fwd(p, p, None, p, p, 1, 8, 4, 4, 8, 0, 0.2, 32, 0, None) == -1 and b"tile" in err()
    assert fwd(p, p + 4, None, p, p, 1, 8, 4, 4, 8, 0, 0.2, 0, 0, None) == -1 and b"aligned" in err()
    assert lib.ffwm_conv3x3_wg_split_weights(p, p, 8, 0, 0, None) == -1
    with pytest.raises(ValueError):
        ops.conv3x3_wg_split(xg, U[:-4].contiguous(), bg, "bias")
    with pytest.raises(ValueError):
        ops.conv3x3_wg_split(xg, U, None, "bias", K=64)
    with pytest.raises(ValueError):
        ops.conv3x3_wg_split(xg, U, bg, "bias", workspace=torch.empty(16, device=DEV))
    with pytest.raises(KeyError):
        ops.conv3x3_wg_split(xg, U, bg, "mfm")
    with pytest.raises(TypeError):
        ops.conv3x3_wg_split(xg.double(), U.double(), bg.double(), "bias")


@pytest.mark.parametrize("case", ws.NONFINITE_CASES)
def test_nonfinite_contract(case):
    from ffwm_amd import ops
    x, w, b, bounds, want = ws.split_nonfinite_case(case)
    U = ops.conv3x3_wg_split_weights(w.cuda())
    for tile in ws.TILES:
        ws.split_nonfinite_check(case, bounds, want, _three(ops, x.cuda(), U, b.cuda(), w.shape[0], tile))


# ---------------------------------------------------------------------------------------------------- the route through the networks
class _Recorder:
    """Wraps ops.conv3x3_wg_split: every call's input, split weights, bias, epilogue, slope and result."""

    def __init__(self, ops):
        self.ops, self.real, self.calls = ops, ops.conv3x3_wg_split, []

    def __enter__(self):
        def wrapped(x, U, bias, epilogue, slope=0.2, out=None, K=None, tile=0, workspace=None):
            y = self.real(x, U, bias, epilogue, slope=slope, out=out, K=K, tile=tile, workspace=workspace)
            self.calls.append((x.detach().clone(), U, bias, epilogue, slope, y.detach().clone()))
            return y
        self.ops.conv3x3_wg_split = wrapped
        return self

    def __exit__(self, *a):
        self.ops.conv3x3_wg_split = self.real


def _run(net, fn):
    """-> (recorded calls, profiler rows, the outputs of fn() cloned)."""
    from ffwm_amd import _lib, ops
    _lib.prof_enable(True)
    _lib.prof_reset()
    try:
        with _Recorder(ops) as rec:
            out = [t.clone() for t in fn()]
            torch.cuda.synchronize()
        rows = _lib.prof_collect()
    finally:
        _lib.prof_enable(False)
    return rec.calls, rows, out


def _check_calls(net, calls, want_epilogues):
    """Every recorded call against the float64 reference of ITS layer on the tensor the network really passed it."""
    names = {U.data_ptr(): n for n, U in net._split_u.items()}
    seen = []
    for x, U, bias, epi, slope, y in calls:
        name = names[U.data_ptr()]
        L = net.layers[name]
        b = torch.zeros(L.w.shape[0]) if bias is None else bias.cpu()
        ws.split_bounds(x.cpu(), L.w.cpu(), b, slope=slope, what="route %s" % name)[epi].check(y)
        assert (bias is None) == (epi == "none")
        seen.append(name)
    assert {c[3] for c in calls} == want_epilogues
    return seen


def _route_checks(net, fn, routed, want_epilogues):
    """First call: the split weights are made, once per routed layer; second call: it reads them; one launch of each of the three
    kernels per routed layer; every call inside its layer's bound."""
    calls, rows, out = _run(net, fn)
    assert sorted(_check_calls(net, calls, want_epilogues)) == sorted(routed) == sorted(net._split_u)
    assert _launches(rows, "conv_wgs_weights") == len(routed)
    for name in ("conv_wgs_in", "conv_wgs_gemm", "conv_wgs_out"):
        assert _launches(rows, name) == len(routed), (name, rows.get(name))
    calls, rows, again = _run(net, fn)
    assert _launches(rows, "conv_wgs_weights") == 0 and len(calls) == len(routed)
    for name in ("conv_wgs_in", "conv_wgs_gemm", "conv_wgs_out"):
        assert _launches(rows, name) == len(routed), (name, rows.get(name))
    assert rows["conv_wgs_gemm"]["launches"] and not any(k.startswith("conv_wg_") for k in rows)          # the fp32 GEMM route is not involved
    for a, b in zip(out, again):
        assert torch.equal(a, b)                                                # no atomics on the way: call to call bit for bit
    return out


def _layer_outputs(folded, x):
    """One forward of a FoldedLightCNN -> the output of every layer (behind its mfm_tail) in order, then fc and the last pool."""
    from ffwm_amd import identity_eval
    outs, real = [], identity_eval._HipExec.layer

    def layer(self, name, x, residual=None, pool=False):
        y = real(self, name, x, residual, pool)
        outs.append(y.clone())
        return y
    identity_eval._HipExec.layer = layer
    try:
        fc, pool = folded(x)
    finally:
        identity_eval._HipExec.layer = real
    return outs + [fc.clone(), pool.clone()]


def _fp32_as_before(make, call, shape, per_layer=False):
    """precision="fp32" is the path as it was: the plan and the launches of an object made without the argument, and its bits.  The
    Winograd kernel's reduction split is capped at two pieces for the comparison (two partial sums meeting in float atomics do not
    depend on the order; four do), and each object's first call is left out: there the vendor's library picks its kernels.
    per_layer (FoldedLightCNN: call returns every layer's output): the vendor's convolution of the 128-channel layers on 4 x 4 planes
    does not reproduce ITSELF from call to call on the MI355X, so the bits are compared layer by layer up to the first layer at
    which the path as it was differs from itself, and that layer has to be one of the vendor's."""
    from ffwm_amd import _lib
    before = _lib.set_option("conv_wino_split", 2)
    try:
        old, new = make(), make(precision="fp32")
        assert old.precision == new.precision == "fp32" and old.plan(*shape) == new.plan(*shape) == new.plan(*shape, precision="fp32")
        call(old), call(new)
        a, again, b = ([t.clone() for t in call(f)] for f in (old, old, new))
        assert old.last_launches == new.last_launches == old.plan(*shape) and not new._split_u and not old._split_u
        n = next((i for i, (p, q) in enumerate(zip(a, again)) if not torch.equal(p, q)), len(a))
        if per_layer:
            convs = [(name, k) for name, k in old.last_launches if k not in ("mfm_tail", "linear", "mfm")]
            print("fp32 path: %d of %d tensors reproduce from call to call%s" % (n, len(a), "" if n == len(a) else ", first not at %s" % (convs[n],)))
            assert n == len(a) or (n >= 8 and convs[n][1] == "vendor_conv")
            assert {k for _, k in convs[:n]} > {"vendor_conv"}                  # the compared part holds own kernels too
        else:
            assert n == len(a), "the fp32 path does not reproduce itself from call to call"
        assert all(torch.equal(p, q) for p, q in zip(a[:n], b[:n]))
    finally:
        _lib.set_option("conv_wino_split", before)


def _small_lightcnn(seed=31):
    """identity_bounds.conditioned_lightcnn with an fc that fits the 2 x 2 x 128 pool of a 32 px input."""
    from ffwm_amd import nets
    net = ib.conditioned_lightcnn(seed)
    torch.manual_seed(seed + 1)
    net.fc = nets.mfm(2 * 2 * 128, 256, type=0)
    with torch.no_grad():
        net.fc.filter.weight.normal_(0, 512 ** -0.5)
        net.fc.filter.bias.zero_()
    return net.eval()


@pytest.fixture(scope="module")
def lightcnn32():
    """The network, its float64 outputs on the CPU (the module path), the input: shared and left unchanged."""
    net = _small_lightcnn()
    x = ib.structured_image(2, 32, 32)
    with torch.no_grad():
        _, fc64, pool64 = copy.deepcopy(net).double()(x.double())
    return net.to(DEV), x.to(DEV), [fc64, pool64]


@pytest.fixture
def every_layer(monkeypatch):
    """32 px keeps these tests quick; planes that small are outside the measured table, so the layers that table excludes
    (identity_eval.SPLIT_EXCLUDED_LAYERS) are opened to the route here, as test_gpu_wino_gemm_bounds opens conv.WG_TABLE."""
    from ffwm_amd import identity_eval
    monkeypatch.setattr(identity_eval, "SPLIT_EXCLUDED_LAYERS", frozenset())


def test_route_through_folded_lightcnn(lightcnn32, every_layer):
    from ffwm_amd.identity_eval import FoldedLightCNN
    net, x, ref = lightcnn32
    folded = FoldedLightCNN(net, precision="bf16x3")
    plan = folded.plan(2, 32, 32)
    routed = [n for n, k in plan if k == "winograd_split"]
    assert len(routed) == 24 and not [k for _, k in plan if k in ("winograd", "conv_mfma")]          # every 3 x 3 layer
    out = _route_checks(folded, lambda: folded(x), routed, {"none"})
    assert folded.last_launches == plan
    # graph replay: the same bits, nothing allocated or transformed inside the capture
    g = FoldedLightCNN(net, graph=True, precision="bf16x3")
    for _ in range(2):
        for a, b in zip(g(x), out):
            assert torch.equal(a, b)
    assert g._graph is not None
    # precision="fp32" is the path as it was: the same plan, launches and bits (the Winograd kernel's reduction split capped at two
    # pieces, where its float atomics do not depend on the order)
    _fp32_as_before(lambda **kw: FoldedLightCNN(net, **kw), lambda f: _layer_outputs(f, x), (2, 32, 32), per_layer=True)


def test_excluded_layers_keep_their_fp32_route():
    """The measured exclusions as they stand, at the size they were measured at: the plan leaves those layers where "fp32" has them,
    and a forward follows the plan."""
    from ffwm_amd import identity_eval
    from ffwm_amd.identity_eval import FoldedLightCNN
    net = ib.conditioned_lightcnn().to(DEV)
    folded = FoldedLightCNN(net, precision="bf16x3")
    plan = folded.plan(1, 128, 128)
    base = {n: k for n, k in FoldedLightCNN(net).plan(1, 128, 128) if k != "mfm_tail"}
    convs = {n: k for n, k in plan if k != "mfm_tail"}
    assert identity_eval.SPLIT_EXCLUDED_LAYERS and all(convs[n] == base[n] != "winograd_split" for n in identity_eval.SPLIT_EXCLUDED_LAYERS)
    assert sum(k == "winograd_split" for k in convs.values()) == 24 - len(identity_eval.SPLIT_EXCLUDED_LAYERS)
    fc, pool = folded(ib.structured_image(1, 128, 128).to(DEV))
    assert folded.last_launches == plan and set(folded._split_u).isdisjoint(identity_eval.SPLIT_EXCLUDED_LAYERS)
    assert fc.shape == (1, 256) and bool(torch.isfinite(fc).all())


def test_folded_lightcnn_end_to_end_against_float64(lightcnn32, every_layer):
    """The project's yardstick for a routed network, 5e-5 (1 + max |ref|) per feature map against the module path in float64 on the CPU
    (test_gpu_wino_gemm_bounds._vs_float64), for both precisions."""
    from ffwm_amd.identity_eval import FoldedLightCNN
    net, x, ref = lightcnn32
    errs = {}
    for precision in ("fp32", "bf16x3"):
        out = FoldedLightCNN(net, precision=precision)(x)
        errs[precision] = [((a.cpu().double() - r).abs().max().item(), 5e-5 * (1 + r.abs().max().item())) for a, r in zip(out, ref)]
        print("FoldedLightCNN %s: max |got - float64| (fc, pool) and the yardstick: %s" % (precision, errs[precision]))
    for precision in ("fp32", "bf16x3"):
        _vs_float64(FoldedLightCNN(net, precision=precision)(x), None, ref, None, precision)


@pytest.fixture(scope="module")
def netg():
    from ffwm_amd import nets
    net = fill.fill_module(nets.FFWM(sn=True, warp_flipcat=torch_refs.warp_flipcat)).to(DEV).eval()
    img = fill.image(1, 3, 32, 32, "netG_in").to(DEV)
    flows = [fill.flow_field(1, s, s, "netG_flow%d" % s).to(DEV) for s in (8, 16, 32)]
    return net, img, flows


def test_route_through_folded_ffwm(netg):
    from ffwm_amd.ffwm_eval import FoldedFFWM
    net, img, flows = netg
    folded = FoldedFFWM(net, precision="bf16x3")
    plan = folded.plan(1, 32, 32)
    routed = [n for n, k in plan if k == "winograd_split"]
    assert len(routed) >= 20 and not [k for _, k in plan if k == "winograd"]
    out = _route_checks(folded, lambda: folded(img, flows, return_att=True), routed, {"bias", "lrelu"})
    assert folded.last_launches == plan
    ref = FoldedFFWM(net)(img, flows, return_att=True)
    for name, a, r in zip(("rec32", "rec64", "rec128", "att"), out, ref):
        d = (a - r).abs().max().item()
        # a figure, not a check: the route is held to its bound call by call above, where the bound is defined
        print("FoldedFFWM bf16x3 against fp32, %s: max |difference| %.3e of max |fp32| %.3e" % (name, d, r.abs().max().item()))
    g = FoldedFFWM(net, graph=True, precision="bf16x3")
    for _ in range(2):
        for a, b in zip(g(img, flows, return_att=True), out):
            assert torch.equal(a, b)
    assert g._graph is not None
    _fp32_as_before(lambda **kw: FoldedFFWM(net, **kw), lambda f: f(img, flows, return_att=True), (1, 32, 32))


def test_face_identifier_top1_under_both_precisions(tmp_path):
    """A gallery of 8 distinct random images, probes taken from it: both precisions return the same top-1 indices."""
    import test_trainer_cpu as T
    import ffwm_amd
    gold, ckpt_dir = T._eval_golden()
    ep = T._prepare_reference_checkpoints(tmp_path, gold, ckpt_dir)
    light = os.path.join(str(tmp_path), "lightcnn_seeded.pth")
    torch.save(ib.conditioned_lightcnn().state_dict(), light)
    gallery = torch.rand(8, 3, 128, 128, generator=torch.Generator().manual_seed(77)).to(DEV)
    probes = gallery[[5, 0, 7, 2]].contiguous()
    top1, feats, fakes = {}, {}, {}
    for precision in ("fp32", "bf16x3"):
        ident = ffwm_amd.FaceIdentifier.from_checkpoints(str(tmp_path), ep, light, ngf=4, device=DEV, graph=False, precision=precision)
        assert ident.precision == ident.front.precision == ident.net.precision == precision
        ident.set_gallery(["%03d" % i for i in range(8)], gallery)
        r = ident(probes)
        kinds = {k for _, k in ident.net.last_launches} | {k for _, k in ident.front.netG.last_launches}
        assert ("winograd_split" in kinds) == (precision == "bf16x3")
        top1[precision], feats[precision], fakes[precision] = r.top_idx[:, 0].cpu(), r.feature.cpu().double(), r.frontal.fake_F128.cpu()
        print("FaceIdentifier %s: top-1 %s, similarities %s" % (precision, top1[precision].tolist(), r.top_sim[:, :2].cpu().tolist()))
    cos = torch.cosine_similarity(feats["fp32"], feats["bf16x3"], dim=1)
    print("max |fake_F128 difference| %.3e, max |feature difference| %.3e, cosine between the features %s"
          % ((fakes["fp32"] - fakes["bf16x3"]).abs().max().item(), (feats["fp32"] - feats["bf16x3"]).abs().max().item(), cos.tolist()))
    assert torch.equal(top1["fp32"], top1["bf16x3"])

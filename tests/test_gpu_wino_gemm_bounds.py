"""Per-element float64 bounds for the batched-GEMM Winograd route of the frozen 3x3 layers (csrc/conv_winograd_gemm.hip): the
three epilogues of the forward, the data gradient with and without the ReLU mask, through BOTH GEMM tiles; and the route itself
through a frozen VGG19 and a frozen LightCNN-29 trunk.  Cases, bounds and their derivation: wino_gemm_cases.py (the CPU restatement
of the same data flow meets them in test_wino_gemm_cpu.py)."""
import pytest
import torch

import conv_bounds as cb
import wino_gemm_cases as wc

pytestmark = pytest.mark.gpu

_IDS = dict(ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))


@pytest.mark.parametrize("tile", wc.TILES)
@pytest.mark.parametrize("kind", cb.FAMILIES)
@pytest.mark.parametrize("shape", wc.SHAPES, **_IDS)
def test_forward_epilogues_per_element(shape, kind, tile):
    from ffwm_amd import ops
    x, w, b, bounds = wc.forward_case(shape, kind)
    K = shape[4]
    xg, bg = x.cuda(), b.cuda()
    U = ops.conv3x3_wg_weights(w.cuda(), False)
    bounds["none"].check(ops.conv3x3_wg(xg, U, None, "none", K=K, tile=tile))
    bounds["relu"].check(ops.conv3x3_wg(xg, U, bg, "relu", tile=tile))
    bounds["mfm"].check(ops.conv3x3_wg(xg, U, bg, "mfm", tile=tile))


@pytest.mark.parametrize("tile", wc.TILES)
@pytest.mark.parametrize("kind", cb.FAMILIES)
@pytest.mark.parametrize("shape", wc.SHAPES, **_IDS)
def test_data_gradient_per_element(shape, kind, tile):
    from ffwm_amd import ops
    go, w, y, bounds = wc.dgrad_case(shape, kind)
    C = shape[1]
    gg = go.cuda()
    U = ops.conv3x3_wg_weights(w.cuda(), True)
    bounds[False].check(ops.conv3x3_wg(gg, U, None, "none", K=C, tile=tile))
    bounds[True].check(ops.conv3x3_wg(gg, U, None, "none", relu_mask=y.cuda(), K=C, tile=tile))


def test_the_plan_reaches_both_tiles_and_arguments_are_checked():
    """The plan takes the 128 x 128 tile exactly when 16 ceil(K / 128) ceil(T / 128) workgroups still cover every compute unit
    (ffwm_conv3x3_wg_tile), and a call without a fixed tile is the call with that tile."""
    from ffwm_amd import _lib, ops
    lib = _lib.load()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    chosen = set()
    for B, C, H, W, K in wc.SHAPES + [(8, 512, 16, 16, 512), (8, 256, 32, 32, 256), (8, 256, 16, 16, 256), (64, 64, 64, 64, 128)]:
        T = B * ((H + 1) // 2) * ((W + 1) // 2)
        want = 128 if 16 * ((K + 127) // 128) * ((T + 127) // 128) >= cus else 64
        assert ops.conv3x3_wg_tile(B, C, H, W, K) == want, (B, C, H, W, K)
        chosen.add(want)
    assert chosen == {64, 128}
    assert ops.conv3x3_wg_tile(0, 8, 4, 4, 8) == 0
    x, w, b, _ = wc.forward_case(wc.SHAPES[3], "iid")
    xg, bg = x.cuda(), b.cuda()
    U = ops.conv3x3_wg_weights(w.cuda(), False)
    assert torch.equal(ops.conv3x3_wg(xg, U, bg, "bias"), ops.conv3x3_wg(xg, U, bg, "bias", tile=ops.conv3x3_wg_tile(*wc.SHAPES[3])))
    p = xg.data_ptr()
    assert lib.ffwm_conv3x3_wg_forward(None, None, None, None, None, 1, 8, 4, 4, 8, 0, None, 0, None) == -1
    assert lib.ffwm_conv3x3_wg_forward(p, p, None, p, p, 1, 8, 4, 4, 8, 7, None, 0, None) == -1 and b"epilogue" in lib.ffwm_last_error()
    assert lib.ffwm_conv3x3_wg_forward(p, p, None, p, p, 1, 8, 4, 4, 8, 0x100, None, 0, None) == -1          # no hidden bits in the epilogue
    assert lib.ffwm_conv3x3_wg_forward(p, p, None, p, p, 1, 8, 4, 4, 7, 3, None, 0, None) == -1 and b"even" in lib.ffwm_last_error()
    assert lib.ffwm_conv3x3_wg_forward(p, p, None, p, p, 1, 8, 4, 4, 8, 0, None, 1, None) == -2
    assert lib.ffwm_conv3x3_wg_forward_tiled(p, p, None, p, p, 1, 8, 4, 4, 8, 0, None, 32, 0, None) == -1 and b"tile" in lib.ffwm_last_error()
    assert lib.ffwm_conv3x3_wg_weights(p, p, 8, 8, 2, 0, None) == -1
    with pytest.raises(ValueError):
        ops.conv3x3_wg(xg, U[:-4].contiguous(), bg, "bias")


# ---------------------------------------------------------------------------------------------------- the route through the networks
class _Recorder:
    """Wraps ops.conv3x3_wg: every call's input, transformed weights, bias, epilogue, mask and result."""

    def __init__(self, ops):
        self.ops, self.real, self.calls = ops, ops.conv3x3_wg, []

    def __enter__(self):
        def wrapped(x, U, bias, epilogue, relu_mask=None, out=None, K=None, tile=0):
            y = self.real(x, U, bias, epilogue, relu_mask=relu_mask, out=out, K=K, tile=tile)
            self.calls.append((x.detach().clone(), U, bias, epilogue, None if relu_mask is None else relu_mask.detach().clone(), y.detach().clone()))
            return y
        self.ops.conv3x3_wg = wrapped
        return self

    def __exit__(self, *a):
        self.ops.conv3x3_wg = self.real


def _check_calls(net, calls):
    """Every recorded call against the float64 reference of ITS layer on ITS input: the per-element bounds of the kernel tests.  (A
    bound for a whole network does not compose from per-layer ones -- a ReLU or a maximum may flip on a last-bit difference -- so
    the route is held to the bound where it is defined: layer by layer, on the tensors the network really passes.)"""
    layers = {}
    for m in net.modules():
        d = m.__dict__.get("_wg_frozen")
        if d is not None:
            layers[d[0].data_ptr()] = (m, False)
            if 1 in d:
                layers[d[1].data_ptr()] = (m, True)
    fwd = dgrad = 0
    for x, U, bias, epi, mask, y in calls:
        m, dg = layers[U.data_ptr()]
        w = m.weight.detach().cpu()
        K, C = w.shape[0], w.shape[1]
        x = x.cpu()
        if dg:
            assert epi == "none" and bias is None
            if mask is not None:
                x = torch.ops.aten.threshold_backward(x, mask.cpu(), 0)
            cb.forward_bound(x, w, None, mode=3, rho=cb.rho_winograd(K), winograd=True, what="route dgrad %d->%d" % (C, K)).check(y)
            dgrad += 1
            continue
        assert mask is None
        rho = cb.rho_winograd(C)
        what = "route fwd %d->%d %s" % (C, K, epi)
        if epi == "none":
            bound = cb.forward_bound(x, w, None, rho=rho, winograd=True, what=what)
        elif epi == "relu":
            bound = wc.relu_bound(cb.forward_bound(x, w, bias.cpu(), rho=rho, winograd=True), what)
        else:
            pre = cb.forward_bound(x, w, bias.cpu(), rho=rho, winograd=True)
            h = K // 2
            bound = cb.Bound(torch.maximum(pre.ref[:, :h], pre.ref[:, h:]), torch.maximum(pre.mag[:, :h], pre.mag[:, h:]), rho, 0.0, False, what)
        bound.check(y)
        fwd += 1
    return fwd, dgrad


def _lightcnn_trunk(net, x):
    """LightCNN29.forward up to pool4 (the fully connected layer behind it needs the 8 x 8 plane of a 128 px input)."""
    x = net.pool1(net.conv1(x))
    x = net.pool2(net.group1(net.block1(x)))
    x = net.pool3(net.group2(net.block2(x)))
    x = net.group3(net.block3(x))
    return net.pool4(net.group4(net.block4(x)))


def _loss(feats):
    return sum(f.square().mean() for f in feats)


def _run(net, fn, x, grad):
    """-> (recorded conv3x3_wg calls, profiler rows, the network's outputs, d(_loss)/dx or None)."""
    from ffwm_amd import _lib, ops
    _lib.prof_enable(True)
    _lib.prof_reset()
    gx = None
    try:
        with _Recorder(ops) as rec:
            if grad:
                x = x.clone().requires_grad_(True)
                out = fn(net, x)
                gx, = torch.autograd.grad(_loss(out), x)
            else:
                with torch.no_grad():
                    out = fn(net, x)
            torch.cuda.synchronize()
        rows = _lib.prof_collect()
    finally:
        _lib.prof_enable(False)
    return rec.calls, rows, out, gx


def _launches(rows, name):
    return rows.get(name, {"launches": 0})["launches"]


def _vs_float64(out, gx, ref_out, ref_gx, what):
    """The network's outputs and its input gradient against the SAME network evaluated through the module path in float64 on the CPU
    (nets.py takes no fused or routed path there).  A per-element bound does not compose through 9-16 layers with ReLU / maximum /
    max-pool selections in between, so this is the yardstick of the sibling test of the large-plane route
    (test_gpu_parity.py::test_vgg_winograd_bias_relu_matches_the_module_path): 5e-5 (1 + max |ref|) per feature map, 1e-4
    (1 + max |ref|) for the input gradient -- fp32 chains of 10^2-10^3 terms per layer err by ~1e-6 of the scale per layer."""
    assert len(out) == len(ref_out)
    for i, (a, r) in enumerate(zip(out, ref_out)):
        assert a.shape == r.shape
        err = (a.detach().cpu().double() - r).abs().max().item()
        assert err <= 5e-5 * (1 + r.abs().max().item()), (what, "output", i, err)
    if gx is not None:
        err = (gx.cpu().double() - ref_gx).abs().max().item()
        assert err <= 1e-4 * (1 + ref_gx.abs().max().item()), (what, "input gradient", err)


@pytest.mark.parametrize("table", ("both", "forward_only"))
@pytest.mark.parametrize("which", ("vgg", "lightcnn"))
def test_route_through_the_frozen_networks(which, table, monkeypatch):
    """Batch 2 at 32 px keeps the test quick; planes that small are outside the measured table (conv.WG_TABLE leaves T <= 40 to the
    vendor), so the table's classes are opened to every T here.  "both": forward and data gradient routed.  "forward_only": the
    data gradient of every class left to the vendor, as the real table leaves 128 -> 256, 96 -> 192 and the small planes of
    256 -> 512 / 512 -> 512 -- the threshold_backward + vendor data gradient branch of the Function's backward."""
    from ffwm_amd import conv, nets
    assert conv._WG, "FFWM_WINOGRAD_GEMM=0 is set: the route under test is off"
    every = (1, 1 << 30)
    monkeypatch.setattr(conv, "WG_TABLE", {ck: (every, every if table == "both" else conv._WG_NEVER) for ck in conv.WG_TABLE})
    torch.manual_seed(3)
    if which == "vgg":
        net = nets.VGG19("relu5_1").cuda().eval()
        ref = nets.VGG19("relu5_1").double().eval()
        x = torch.rand(2, 3, 32, 32, device="cuda")
        fn = lambda n, t: list(n(t).values())
    else:
        net = nets.LightCNN29().cuda().eval()
        ref = nets.LightCNN29().double().eval()
        for p in net.parameters():
            p.requires_grad = False
        x = torch.rand(2, 1, 32, 32, device="cuda")
        fn = lambda n, t: [_lightcnn_trunk(n, t)]
    ref.load_state_dict({k: v.double().cpu() for k, v in net.state_dict().items()})
    xr = x.double().cpu().requires_grad_(True)
    ref_out = fn(ref, xr)
    ref_gx, = torch.autograd.grad(_loss(ref_out), xr)
    ref_out = [r.detach() for r in ref_out]

    calls, rows, out, gx = _run(net, fn, x, True)          # first call: the transforms are made, eagerly, once per layer and direction
    _vs_float64(out, gx, ref_out, ref_gx, "first call")
    routed = sum(1 for m in net.modules() if "_wg_frozen" in m.__dict__)
    assert routed >= 3
    assert _launches(rows, "conv_wg_weights") == (2 if table == "both" else 1) * routed
    fwd, dgrad = _check_calls(net, calls)
    assert fwd == routed and dgrad == (routed if table == "both" else 0)
    for name in ("conv_wg_in", "conv_wg_gemm", "conv_wg_out"):
        assert _launches(rows, name) == fwd + dgrad, (name, rows.get(name))
    calls, rows, out, gx = _run(net, fn, x, True)          # second call: reads them
    _vs_float64(out, gx, ref_out, ref_gx, "second call")
    assert _launches(rows, "conv_wg_weights") == 0 and _launches(rows, "conv_wg_gemm") == fwd + dgrad
    calls, rows, out, _ = _run(net, fn, x, False)          # no gradient: the fused epilogues (LightCNN: bias + max-feature-map)
    _vs_float64(out, None, ref_out, None, "no gradient")
    assert _launches(rows, "conv_wg_weights") == 0
    assert _check_calls(net, calls) == (routed, 0)
    assert {c[3] for c in calls} == ({"relu"} if which == "vgg" else {"mfm"})
    # a trainable weight sends its layer back to the old route
    layer = next(m for m in net.modules() if "_wg_frozen" in m.__dict__)
    layer.weight.requires_grad_(True)
    calls, rows, out, _ = _run(net, fn, x, False)
    _vs_float64(out, None, ref_out, None, "one layer on the old route")
    assert len(calls) == routed - 1 and layer.__dict__["_wg_frozen"][0].data_ptr() not in {c[1].data_ptr() for c in calls}


def test_route_with_the_measured_table():
    """conv.WG_TABLE as it stands, on a plane inside its ranges: VGG19's relu3 / relu4 stack fed a 64 x 64 plane, batch 2: 32 x 32 and 16 x 16 behind the pools
    (T = 512 and 128) -- conv3_1 (128 -> 256: forward routed, data gradient the vendor's), conv3_2-4 (both routed), conv4_1 and
    conv4_2 at T = 128 (forward routed, data gradient the vendor's) -- features and input gradient against float64."""
    from ffwm_amd import conv, nets
    assert conv._WG
    torch.manual_seed(5)
    vgg = nets.VGG19("relu4_2").cuda().eval()
    ref = nets.VGG19("relu4_2").double().eval()
    ref.load_state_dict({k: v.double().cpu() for k, v in vgg.state_dict().items()})
    names = vgg.slices[vgg.slices.index("relu3_1"):]

    def tail(n, t):
        # the slices from relu3_1 on, through VGG19.forward's own loop: a network whose `slices` start there
        saved, n.slices = n.slices, names
        try:
            return list(n(t).values())
        finally:
            n.slices = saved
    x = torch.rand(2, 128, 64, 64, device="cuda")
    xr = x.double().cpu().requires_grad_(True)
    ref_out = tail(ref, xr)
    ref_gx, = torch.autograd.grad(_loss(ref_out), xr)
    calls, rows, out, gx = _run(vgg, tail, x, True)
    _vs_float64(out, gx, [r.detach() for r in ref_out], ref_gx, "measured table")
    fwd, dgrad = _check_calls(vgg, calls)
    assert (fwd, dgrad) == (6, 3), (fwd, dgrad)            # forward: conv3_1-4, conv4_1-2; data gradient: conv3_2-4 only

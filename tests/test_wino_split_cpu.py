"""The split batched-GEMM Winograd route (csrc/conv_winograd_gemm_split.hip) without a GPU: a torch restatement of its data flow
(wino_split_cases.split_flow_f32) meets the per-element bounds with SAFETY = 1 and the exact family bit for bit, every mutant of it
misses the exact family; the library exports the entry points, answers the size queries and refuses bad arguments before any launch;
and the `precision` option of the folded networks: "fp32" is the plan as it was, "bf16x3" lists `winograd_split` for exactly the
layers the predicate names."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import conv_bounds as cb  # noqa: E402
import fill  # noqa: E402
import wino_split_cases as ws  # noqa: E402

_IDS = dict(ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("kind", cb.FAMILIES)
@pytest.mark.parametrize("shape", ws.SHAPES, **_IDS)
def test_restatement_meets_the_bounds_with_safety_one(shape, kind):
    x, w, b, bounds = ws.split_case(shape, kind)
    rho1 = ws.rho_split(shape[1], safety=1.0)
    for epi in ws.EPILOGUES:
        bd = bounds[epi]
        saved, bd.post = bd.post, bd.post - cb.SAFETY + 1.0          # SAFETY = 1 on the |ref| term too
        try:
            bd.check(ws.split_flow_f32(x, w, b, epi), rho=rho1)
        finally:
            bd.post = saved


def test_bound_constants():
    assert ws.rho_split(64) == 16 * (2.0 ** -16 * (1 + 2.0 ** -6) + 4 * (3 * 64 + 11) * 2.0 ** -24 * (1 + 2.0 ** -6))
    assert 1.0e-3 < ws.rho_split(64) < 1.1e-3 and 4.3e-4 < ws.rho_split(64, 1.0) < 4.5e-4
    with pytest.raises(ValueError):
        ws.split_bounds(torch.full((1, 32, 2, 2), 2.0 ** 125), torch.ones(32, 32, 3, 3), torch.zeros(32))


def test_exact_family_and_its_mutants():
    x, w = ws.split_exact_inputs()
    three, full, hh = ws.split_exact_reference(x, w)
    assert bool((three != full).any()) and bool((three != hh).any())
    assert torch.equal(ws.split_flow_f32(x, w), three.float())
    for mutant in ws.MUTANTS:
        assert not torch.equal(ws.split_flow_f32(x, w, mutant=mutant), three.float()), mutant
    # the bound alone would let two of them pass: that is what the family is for
    bound = ws.split_bounds(x, w, torch.zeros(w.shape[0]))["none"]
    assert bound.measure(ws.split_flow_f32(x, w, mutant="lo_lo_added"))[0] <= 1.0


@pytest.mark.parametrize("case", ws.NONFINITE_CASES)
def test_nonfinite_contract_of_the_restatement(case):
    x, w, b, bounds, want = ws.split_nonfinite_case(case)
    ws.split_nonfinite_check(case, bounds, want, {epi: ws.split_flow_f32(x, w, b, epi) for epi in ws.EPILOGUES})


# ---------------------------------------------------------------------------------------------------- the library
@pytest.fixture(scope="module")
def hiplib():
    from ffwm_amd import build, _lib
    build.build()
    return _lib.load()


def test_symbols_sizes_and_argument_errors(hiplib):
    from ffwm_amd import ffwm_eval
    for name in ("ffwm_conv3x3_wg_split_weights_bytes", "ffwm_conv3x3_wg_split_workspace_bytes", "ffwm_conv3x3_wg_split_weights",
                 "ffwm_conv3x3_wg_split_tile", "ffwm_conv3x3_wg_split_forward"):
        assert hasattr(hiplib, name), name
    assert hiplib.ffwm_abi_version() == 5
    # U: a hi and a lo bf16 per entry, C rounded up to 32; the workspace: V of the same 4 bytes per entry and fp32 M, the 128 tile's padding
    assert hiplib.ffwm_conv3x3_wg_split_weights_bytes(70, 19) == 16 * 32 * 70 * 4
    assert hiplib.ffwm_conv3x3_wg_split_weights_bytes(64, 64) == 16 * 64 * 64 * 4
    assert hiplib.ffwm_conv3x3_wg_split_weights_bytes(0, 8) == 0
    assert hiplib.ffwm_conv3x3_wg_split_workspace_bytes(2, 19, 7, 9, 70) == 16 * 128 * (32 + 128) * 4
    assert hiplib.ffwm_conv3x3_wg_split_workspace_bytes(2, 130, 12, 12, 200) == 16 * 128 * (160 + 256) * 4
    assert hiplib.ffwm_conv3x3_wg_split_workspace_bytes(1, 8, 0, 4, 8) == 0
    for shape in ws.SHAPES + [(8, 195, 128, 128, 195), (1, 64, 64, 64, 64)]:
        assert hiplib.ffwm_conv3x3_wg_split_workspace_bytes(*shape) == ffwm_eval.split_workspace_bytes(*shape), shape
    assert ffwm_eval.split_workspace_bytes(8, 195, 128, 128, 195) > 400e6 > ffwm_eval.SPLIT_WORKSPACE_LIMIT == 256 << 20
    assert hiplib.ffwm_conv3x3_wg_split_tile(0, 8, 4, 4, 8) == 0

    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value // 16 * 16 + 16
    fwd, err = hiplib.ffwm_conv3x3_wg_split_forward, hiplib.ffwm_last_error
    assert fwd(None, None, None, None, None, 1, 8, 4, 4, 8, 0, 0.2, 0, 0, None) == -1 and b"NULL" in err()
    assert fwd(p, p, None, p, p, 1, 8, 4, 0, 8, 0, 0.2, 0, 0, None) == -1 and b"positive" in err()
    assert fwd(p, p, p, p, p, 1, 8, 4, 4, 8, 3, 0.2, 0, 0, None) == -1 and b"epilogue" in err()          # no mfm, no relu here
    assert fwd(p, p, p, p, p, 1, 8, 4, 4, 8, 0x100, 0.2, 0, 0, None) == -1 and b"epilogue" in err()      # no hidden bits
    assert fwd(p, p, None, p, p, 1, 8, 4, 4, 8, 1, 0.2, 0, 0, None) == -1 and b"bias" in err()
    assert fwd(p, p, None, p, p, 1, 8, 4, 4, 8, 0, 0.2, 32, 0, None) == -1 and b"tile" in err()
    assert fwd(p, p + 4, None, p, p, 1, 8, 4, 4, 8, 0, 0.2, 0, 0, None) == -1 and b"aligned" in err()
    assert fwd(p, p, None, p, p + 8, 1, 8, 4, 4, 8, 0, 0.2, 0, 0, None) == -1 and b"aligned" in err()
    assert fwd(p, p, None, p, p, 1, 8, 4, 4, 8, 0, 0.2, 0, 1, None) == -2 and b"float32" in err()
    assert fwd(p, p, None, p, p, 1 << 12, 1 << 10, 1 << 5, 1 << 5, 8, 0, 0.2, 0, 0, None) == -3
    wts = hiplib.ffwm_conv3x3_wg_split_weights
    assert wts(None, p, 8, 8, 0, None) == -1 and b"NULL" in err()
    assert wts(p, p, 0, 8, 0, None) == -1
    assert wts(p, p + 4, 8, 8, 0, None) == -1 and b"aligned" in err()
    assert wts(p, p, 8, 8, 1, None) == -2
    assert wts(p, p, 1 << 16, 1 << 16, 0, None) == -3


# ---------------------------------------------------------------------------------------------------- the option
@pytest.fixture(scope="module")
def folded():
    from ffwm_amd import nets
    from ffwm_amd.ffwm_eval import FoldedFFWM
    from ffwm_amd.identity_eval import FoldedLightCNN
    import torch_refs
    return (FoldedFFWM(fill.fill_module(nets.FFWM(sn=True, warp_flipcat=torch_refs.warp_flipcat)).eval(), backend="torch"),
            FoldedLightCNN(fill.fill_module(nets.LightCNN29()).eval()))


def _conv_shapes(net, B, H, W):
    """{layer name: the _Spec its convolution sees}, through the plan executor."""
    seen = {}
    route = net._route

    def spy(name, x, *a):
        seen[name] = x
        return route(name, x, *a)
    net._route = spy
    try:
        net.plan(B, H, W)
    finally:
        del net._route
    return seen


@pytest.mark.parametrize("which,shape", [(0, (1, 128, 128)), (0, (8, 128, 128)), (0, (1, 32, 32)), (1, (1, 128, 128)), (1, (8, 128, 128))])
def test_plans_of_the_precisions(folded, which, shape):
    from ffwm_amd import ffwm_eval, identity_eval
    net = folded[which]
    mod = (ffwm_eval, identity_eval)[which]
    assert "winograd_split" in mod.KINDS and mod.SPLIT_EXCLUDED_LAYERS <= set(net.layers)
    base = net.plan(*shape)
    assert net.plan(*shape, precision="fp32") == base and not any(k == "winograd_split" for _, k in base)
    split = net.plan(*shape, precision="bf16x3")
    assert net.precision == "fp32" and net.plan(*shape) == base          # the argument leaves the object as it was
    specs = _conv_shapes(net, *shape)
    named = {n for n, x in specs.items() if n not in mod.SPLIT_EXCLUDED_LAYERS and not n.endswith(".input")
             and ffwm_eval.split_route_ok(net.layers[n], x)}
    for n in named:
        L = net.layers[n]
        assert (L.k, L.stride, L.pad) == (3, 1, 1) and min(L.w.shape[0], L.w.shape[1]) >= 32
        assert ffwm_eval.split_workspace_bytes(specs[n].shape[0], L.w.shape[1], specs[n].shape[2], specs[n].shape[3], L.w.shape[0]) <= 256 << 20
    assert named and {n for n, k in split if k == "winograd_split"} == named
    # every other entry unchanged: the split plan is the base plan with the named layers' convolution launches replaced (FoldedFFWM: a
    # vendor convolution's bias_act launch goes with it)
    it = iter(split)
    for n, k in base:
        if n in named and k in ("winograd", "conv_mfma", "vendor_conv"):
            assert next(it) == (n, "winograd_split")
        elif n in named and which == 0 and k == "bias_act":
            continue
        else:
            assert next(it) == (n, k)
    assert next(it, None) is None
    assert set(k for _, k in split) <= set(mod.KINDS)
    if which == 0 and shape[0] == 8:          # the memory condition: netG's 195-channel layers at 128 x 128, batch 8 keep the fused kernel
        big = {n for n, x in specs.items() if x.shape[2] == 128 and net.layers[n].k == 3 and net.layers[n].w.shape[1] >= 128}
        assert big and not (big & named)
    if which == 1:                            # the layers pinned to the vendor under fp32 are among those the split route reaches
        assert identity_eval.VENDOR_LAYERS - mod.SPLIT_EXCLUDED_LAYERS <= named


def test_precision_is_checked(folded):
    from ffwm_amd import nets
    from ffwm_amd.ffwm_eval import FoldedFFWM, Frontalizer
    from ffwm_amd.identity_eval import FaceIdentifier, FoldedLightCNN
    light = fill.fill_module(nets.LightCNN29()).eval()
    assert folded[0].precision == folded[1].precision == "fp32"
    with pytest.raises(ValueError, match="torch backend"):
        FoldedLightCNN(light, precision="bf16x3")
    with pytest.raises(ValueError, match="torch backend"):
        FoldedLightCNN(light, backend="torch", precision="bf16x3")
    with pytest.raises(ValueError, match="precision must be"):
        FoldedLightCNN(light, precision="fp16")
    with pytest.raises(ValueError, match="precision must be"):
        folded[1].plan(1, 128, 128, precision="bf16")
    import torch_refs
    netG = fill.fill_module(nets.FFWM(sn=True, warp_flipcat=torch_refs.warp_flipcat)).eval()
    flow = nets.FlowNet(4).eval()
    with pytest.raises(ValueError, match="torch backend"):
        FoldedFFWM(netG, backend="torch", precision="bf16x3")
    with pytest.raises(ValueError, match="torch backend"):
        Frontalizer(flow, netG, graph=False, backend="torch", precision="bf16x3")
    with pytest.raises(ValueError, match="torch backend"):
        FaceIdentifier(flow, netG, light, graph=False, backend="torch", precision="bf16x3")
    assert Frontalizer(flow, netG, graph=False, backend="torch", precision="fp32").precision == "fp32"

"""The split batched-GEMM Winograd route as the train step's frozen loss networks use it, on the GPU (ffwm_conv3x3_wg_split_apply,
ffwm_conv3x3_wg_split_weights_dgrad, ops.conv3x3_wg_split_frozen, conv.WGS_TABLE, FFWMTrainer(loss_precision="bf16x3")): per-element
float64 bounds of the data gradient (plain and behind a ReLU mask) and of the four epilogues through both GEMM tiles, the exact family
through the data gradient bit for bit, determinism, the argument checks, the non-finite contract; the route through a frozen VGG19
and a frozen LightCNN-29 trunk call by call, with the launch counts; a captured forward + backward; one trainer step per precision.
Cases, bounds and their derivation: wino_split_train_cases.py."""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import conv_bounds as cb  # noqa: E402
import wino_split_cases as ws  # noqa: E402
import wino_split_train_cases as wt  # noqa: E402
from test_gpu_wino_gemm_bounds import _launches, _lightcnn_trunk, _loss, _vs_float64  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

_IDS = dict(ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))


# ---------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("tile", wt.TILES)
@pytest.mark.parametrize("kind", cb.FAMILIES)
@pytest.mark.parametrize("shape", wt.DGRAD_SHAPES, **_IDS)
def test_data_gradient_per_element(shape, kind, tile):
    from ffwm_amd import ops
    go, w, y, bounds = wt.split_dgrad_case(shape, kind)
    C = shape[1]
    gg, yg = go.cuda(), y.cuda()
    U = ops.conv3x3_wg_split_weights(w.cuda(), data_gradient=True)
    bounds[False].check(ops.conv3x3_wg_split_frozen(gg, U, None, "none", K=C, tile=tile))
    masked = ops.conv3x3_wg_split_frozen(gg, U, None, "none", relu_mask=yg, K=C, tile=tile)
    bounds[True].check(masked)
    # the mask is an exact selection made in front of the transform: the unmasked call on threshold_backward's result, bit for bit
    plain = ops.conv3x3_wg_split_frozen(torch.ops.aten.threshold_backward(gg, yg, 0), U, None, "none", K=C, tile=tile)
    assert torch.equal(masked.nan_to_num(nan=1.5e38), plain.nan_to_num(nan=1.5e38))


@pytest.mark.parametrize("tile", wt.TILES)
@pytest.mark.parametrize("kind", cb.FAMILIES)
@pytest.mark.parametrize("shape", wt.SHAPES, **_IDS)
def test_epilogues_per_element(shape, kind, tile):
    from ffwm_amd import ops
    x, w, b, bounds = wt.split_forward_case(shape, kind)
    K = shape[4]
    xg, bg = x.cuda(), b.cuda()
    U = ops.conv3x3_wg_split_weights(w.cuda())
    got = {"none": ops.conv3x3_wg_split_frozen(xg, U, None, "none", K=K, tile=tile)}
    for epi in ("bias", "relu", "mfm"):
        got[epi] = ops.conv3x3_wg_split_frozen(xg, U, bg, epi, tile=tile)
    for epi in wt.EPILOGUES:
        bounds[epi].check(got[epi])
    # the inference entry's value, and the epilogues as ATen applies them to it (NaN stays NaN, -inf gives 0; maximum's NaN rule)
    assert torch.equal(got["bias"].nan_to_num(nan=1.5e38), ops.conv3x3_wg_split(xg, U, bg, "bias", tile=tile).nan_to_num(nan=1.5e38))
    assert torch.equal(got["relu"].nan_to_num(nan=1.5e38), torch.relu(got["bias"]).nan_to_num(nan=1.5e38))
    assert got["mfm"].shape == (shape[0], K // 2, shape[2], shape[3])
    assert torch.equal(got["mfm"].nan_to_num(nan=1.5e38), torch.maximum(got["bias"][:, :K // 2], got["bias"][:, K // 2:]).nan_to_num(nan=1.5e38))


@pytest.mark.parametrize("shape", wt.DGRAD_SHAPES, **_IDS)
def test_data_gradient_weights_are_the_transposed_rotated_forward_weights(shape):
    from ffwm_amd import ops
    _, w, _, _ = wt.split_dgrad_case(shape, "iid")
    wg = w.cuda()
    U = ops.conv3x3_wg_split_weights(wg, data_gradient=True)
    assert U.numel() * 4 == wt.weights_bytes(shape[1], shape[4])
    assert torch.equal(U.view(torch.int32), ops.conv3x3_wg_split_weights(wg.transpose(0, 1).flip(2, 3).contiguous()).view(torch.int32))
    assert torch.equal(ops.conv3x3_wg_split_weights(wg, data_gradient=False).view(torch.int32), ops.conv3x3_wg_split_weights(wg).view(torch.int32))


@pytest.mark.parametrize("tile", wt.TILES)
def test_exact_family_through_the_data_gradient_bit_for_bit(tile):
    from ffwm_amd import ops
    go, w, three, full, hh = wt.exact_dgrad_inputs()
    U = ops.conv3x3_wg_split_weights(w.cuda(), data_gradient=True)
    got = ops.conv3x3_wg_split_frozen(go.cuda(), U, None, "none", K=w.shape[1], tile=tile).cpu()
    assert not torch.equal(three.float(), hh.float()) and not torch.equal(three.float(), full.float())
    bad = (got != three.float()).nonzero()
    assert bad.shape[0] == 0, "%d elements differ from the three-term value, first at %s" % (bad.shape[0], tuple(int(i) for i in bad[0]))
    assert not torch.equal(got, hh.float()) and not torch.equal(got, full.float())


@pytest.mark.parametrize("tile", wt.TILES)
def test_two_calls_agree_bit_for_bit(tile):
    from ffwm_amd import ops
    shape = wt.DGRAD_SHAPES[4]
    go, w, y, _ = wt.split_dgrad_case(shape, "iid")
    x, wf, b, _ = wt.split_forward_case(shape, "iid")
    gg, yg, xg, bg = go.cuda(), y.cuda(), x.cuda(), b.cuda()
    Ub, Uf = ops.conv3x3_wg_split_weights(w.cuda(), data_gradient=True), ops.conv3x3_wg_split_weights(wf.cuda())
    assert torch.equal(Ub.view(torch.int32), ops.conv3x3_wg_split_weights(w.cuda(), data_gradient=True).view(torch.int32))

    def all_of_them():
        return [ops.conv3x3_wg_split_frozen(gg, Ub, None, "none", relu_mask=yg, K=shape[1], tile=tile)] + [
            ops.conv3x3_wg_split_frozen(xg, Uf, bg, epi, tile=tile) for epi in ("bias", "relu", "mfm")]
    for a, again in zip(all_of_them(), all_of_them()):
        assert torch.equal(a.nan_to_num(nan=1.5e38), again.nan_to_num(nan=1.5e38))


def test_arguments_are_checked():
    from ffwm_amd import _lib, ops
    lib = _lib.load()
    shape = wt.SHAPES[3]
    x, w, b, _ = wt.split_forward_case(shape, "iid")
    xg, bg = x.cuda(), b.cuda()
    U = ops.conv3x3_wg_split_weights(w.cuda())
    assert torch.equal(ops.conv3x3_wg_split_frozen(xg, U, bg, "relu"),
                       ops.conv3x3_wg_split_frozen(xg, U, bg, "relu", tile=ops.conv3x3_wg_split_tile(*shape)))
    out = torch.empty(1, 32, 32, 32, device=DEV)
    assert ops.conv3x3_wg_split_frozen(xg, U, bg, "mfm", out=out) is out
    p = xg.data_ptr()
    run, err = lib.ffwm_conv3x3_wg_split_apply, lib.ffwm_last_error
    assert run(None, None, None, None, None, 1, 8, 4, 4, 8, 0, None, 0, 0, None) == -1 and b"NULL" in err()
    assert run(p, p, None, p, None, 1, 8, 4, 4, 8, 0, None, 0, 0, None) == -1 and b"NULL" in err()
    assert run(p, p, p, p, p, 1, 8, 4, 4, 8, 4, None, 0, 0, None) == -1 and b"epilogue" in err()
    assert run(p, p, p, p, p, 1, 8, 4, 4, 8, 0x100, None, 0, 0, None) == -1 and b"epilogue" in err()          # no hidden bits in the epilogue
    assert run(p, p, None, p, p, 1, 8, 4, 4, 8, 2, None, 0, 0, None) == -1 and b"bias" in err()
    assert run(p, p, p, p, p, 1, 8, 4, 4, 7, 3, None, 0, 0, None) == -1 and b"even" in err()
    assert run(p, p + 4, None, p, p, 1, 8, 4, 4, 8, 0, None, 0, 0, None) == -1 and b"aligned" in err()
    assert run(p, p, None, p, p, 1, 8, 4, 4, 8, 0, None, 32, 0, None) == -1 and b"tile" in err()
    assert run(p, p, None, p, p, 1, 8, 4, 4, 8, 0, None, 0, 1, None) == -2
    assert lib.ffwm_conv3x3_wg_split_weights_dgrad(p, p, 8, 0, 0, None) == -1
    assert lib.ffwm_conv3x3_wg_split_weights_dgrad(p, p + 4, 8, 8, 0, None) == -1 and b"aligned" in err()
    with pytest.raises(ValueError):
        ops.conv3x3_wg_split_frozen(xg, U[:-4].contiguous(), bg, "bias")
    with pytest.raises(ValueError):
        ops.conv3x3_wg_split_frozen(xg, U, None, "relu", K=64)
    with pytest.raises(ValueError):
        ops.conv3x3_wg_split_frozen(xg, U, bg, "bias", workspace=torch.empty(16, device=DEV))
    with pytest.raises(ValueError):
        ops.conv3x3_wg_split_frozen(xg, U, bg, "bias", relu_mask=xg[:, :8].contiguous())
    with pytest.raises(KeyError):
        ops.conv3x3_wg_split_frozen(xg, U, bg, "lrelu")
    with pytest.raises(TypeError):
        ops.conv3x3_wg_split_frozen(xg.double(), U.double(), bg.double(), "bias")
    # the inference entry keeps its refusals
    assert lib.ffwm_conv3x3_wg_split_forward(p, p, p, p, p, 1, 8, 4, 4, 8, 3, 0.2, 0, 0, None) == -1 and b"epilogue" in err()
    with pytest.raises(KeyError):
        ops.conv3x3_wg_split(xg, U, bg, "mfm")


@pytest.mark.parametrize("case", ws.NONFINITE_CASES)
def test_nonfinite_contract(case):
    from ffwm_amd import ops
    x, w, b, bounds, want = ws.split_nonfinite_case(case)
    U = ops.conv3x3_wg_split_weights(w.cuda())
    xg, bg = x.cuda(), b.cuda()
    for tile in wt.TILES:
        outs = {"none": ops.conv3x3_wg_split_frozen(xg, U, None, "none", K=w.shape[0], tile=tile),
                "bias": ops.conv3x3_wg_split_frozen(xg, U, bg, "bias", tile=tile)}
        ws.split_nonfinite_check(case, {k: bounds[k] for k in outs}, want, outs)
        if case == "nan_weight":
            continue
        # a NaN or an infinity behind a zero of the mask does not reach the result
        _, _, _, mask, bound = wt.nonfinite_masked_case(case)
        got = ops.conv3x3_wg_split_frozen(xg, U, None, "none", relu_mask=mask.cuda(), K=w.shape[0], tile=tile)
        assert bool(torch.isfinite(got).all())
        bound.check(got)


# ---------------------------------------------------------------------------------------------------- the route through the networks
class _Recorder:
    """Wraps ops.conv3x3_wg_split_frozen: every call's input, split weights, bias, epilogue, mask and result."""

    def __init__(self, ops):
        self.ops, self.real, self.calls = ops, ops.conv3x3_wg_split_frozen, []

    def __enter__(self):
        def wrapped(x, U, bias, epilogue, relu_mask=None, out=None, K=None, tile=0, workspace=None):
            y = self.real(x, U, bias, epilogue, relu_mask=relu_mask, out=out, K=K, tile=tile, workspace=workspace)
            self.calls.append((x.detach().clone(), U, bias, epilogue, None if relu_mask is None else relu_mask.detach().clone(), y.detach().clone()))
            return y
        self.ops.conv3x3_wg_split_frozen = wrapped
        return self

    def __exit__(self, *a):
        self.ops.conv3x3_wg_split_frozen = self.real


def _check_calls(net, calls):
    """Every recorded call against the float64 bound of ITS layer on the tensors the network really passed it -> (forward calls,
    data-gradient calls)."""
    layers = {}
    for m in net.modules():
        d = m.__dict__.get("_wg_frozen")
        if d is not None:
            for direction in (0, 1):
                if "s%d" % direction in d:
                    layers[d["s%d" % direction].data_ptr()] = (m, bool(direction))
    fwd = dgrad = 0
    for x, U, bias, epi, mask, y in calls:
        m, dg = layers[U.data_ptr()]
        w = m.weight.detach()
        assert not dg or (epi == "none" and bias is None)
        assert dg or mask is None
        wt.route_bound(x, w, bias, epi, mask, dg, what="route %s %d->%d %s" % ("dgrad" if dg else "fwd", w.shape[1], w.shape[0], epi)).check(y)
        fwd, dgrad = fwd + (not dg), dgrad + dg
    return fwd, dgrad


def _run(net, fn, x, grad):
    """-> (recorded conv3x3_wg_split_frozen calls, profiler rows, the network's outputs, d(_loss)/dx or None)."""
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


def _open_tables(monkeypatch, conv, table):
    """conv.WGS_TABLE with the classes of conv.WG_TABLE opened to every T (the planes of a 32 px input are outside every measured
    range): "both" directions, or "forward_only" (the data gradient left where "fp32" has it: at these T, the vendor)."""
    every = (1, 1 << 30)
    monkeypatch.setattr(conv, "WGS_TABLE", {ck: (every, every if table == "both" else conv._WG_NEVER) for ck in conv.WG_TABLE})


@pytest.mark.parametrize("table", ("both", "forward_only"))
@pytest.mark.parametrize("which", ("vgg", "lightcnn"))
def test_route_through_the_frozen_networks(which, table, monkeypatch):
    """test_gpu_wino_gemm_bounds.test_route_through_the_frozen_networks under wg_set_precision(net, "bf16x3"): batch 2 at 32 px, every
    routed call inside its own layer's bound, the launch counts, the fused epilogues without a gradient, outputs and input gradient
    against the float64 module path with that test's yardstick."""
    from ffwm_amd import conv, nets
    assert conv._WG, "FFWM_WINOGRAD_GEMM=0 is set: the route under test is off"
    _open_tables(monkeypatch, conv, table)
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
    conv.wg_set_precision(net, "bf16x3")
    ref.load_state_dict({k: v.double().cpu() for k, v in net.state_dict().items()})
    xr = x.double().cpu().requires_grad_(True)
    ref_out = fn(ref, xr)
    ref_gx, = torch.autograd.grad(_loss(ref_out), xr)
    ref_out = [r.detach() for r in ref_out]
    dirs = 2 if table == "both" else 1

    calls, rows, out, gx = _run(net, fn, x, True)          # first call: the transforms are made, eagerly, once per layer and direction
    routed = sum(1 for m in net.modules() if "_wg_frozen" in m.__dict__)
    assert routed >= 3
    assert _launches(rows, "conv_wgs_weights") == dirs * routed
    fwd, dgrad = _check_calls(net, calls)
    assert fwd == routed and dgrad == (routed if table == "both" else 0)
    for name in ("conv_wgs_in", "conv_wgs_gemm", "conv_wgs_out"):
        assert _launches(rows, name) == fwd + dgrad, (name, rows.get(name))
    assert not any(_launches(rows, name) for name in ("conv_wg_in", "conv_wg_gemm", "conv_wg_out"))          # no fp32 GEMM for a split-routed layer
    # no fp32 U either for a direction whose whole WG_TABLE range went to the split route ("forward_only": the class's fp32 data
    # gradient keeps its U for the T at which WG_TABLE routes it)
    fp32_u = 0
    for m in net.modules():
        d = m.__dict__.get("_wg_frozen")
        if d is not None:
            keep = [1] if table == "forward_only" and conv._wg_class(m.weight)[1] != conv._WG_NEVER else []
            assert [k for k in d if k != "key" and not isinstance(k, str)] == keep
            assert sorted(k for k in d if isinstance(k, str) and k != "key") == ["s0", "s1"][:dirs]
            fp32_u += len(keep)
    assert _launches(rows, "conv_wg_weights") == fp32_u
    _vs_float64(out, gx, ref_out, ref_gx, "first call")
    calls, rows, out, gx = _run(net, fn, x, True)          # second call: reads them
    _vs_float64(out, gx, ref_out, ref_gx, "second call")
    assert _launches(rows, "conv_wgs_weights") == 0 and _launches(rows, "conv_wgs_gemm") == fwd + dgrad
    calls, rows, out, _ = _run(net, fn, x, False)          # no gradient: the fused epilogues (LightCNN: bias + max-feature-map)
    _vs_float64(out, None, ref_out, None, "no gradient")
    assert _launches(rows, "conv_wgs_weights") == 0
    assert _check_calls(net, calls) == (routed, 0)
    assert {c[3] for c in calls} == ({"relu"} if which == "vgg" else {"mfm"})
    # a trainable weight sends its layer back to the route it had
    layer = next(m for m in net.modules() if "_wg_frozen" in m.__dict__)
    layer.weight.requires_grad_(True)
    calls, rows, out, _ = _run(net, fn, x, False)
    _vs_float64(out, None, ref_out, None, "one layer on the old route")
    assert len(calls) == routed - 1 and layer.__dict__["_wg_frozen"]["s0"].data_ptr() not in {c[1].data_ptr() for c in calls}


def test_fp32_stamp_and_layers_outside_the_table_keep_their_route(monkeypatch):
    """Two networks in one process differ: the one stamped "fp32" (or never stamped) runs conv_wg_gemm where WG_TABLE says so and no
    split kernel, with WGS_TABLE open; under "bf16x3" a class outside WGS_TABLE keeps the fp32 GEMM route."""
    from ffwm_amd import conv, nets
    every = (1, 1 << 30)
    monkeypatch.setattr(conv, "WG_TABLE", {ck: (every, every) for ck in conv.WG_TABLE})
    monkeypatch.setattr(conv, "WGS_TABLE", {(256, 256): (every, every)})
    torch.manual_seed(4)
    x = torch.rand(2, 3, 32, 32, device="cuda")
    fn = lambda n, t: list(n(t).values())
    plain, split = nets.VGG19("relu5_1").cuda().eval(), nets.VGG19("relu5_1").cuda().eval()
    split.load_state_dict(plain.state_dict())
    conv.wg_set_precision(split, "bf16x3")
    _, rows_plain, out_plain, gx_plain = _run(plain, fn, x, True)
    calls, rows, out, gx = _run(split, fn, x, True)
    n_fp32 = _launches(rows_plain, "conv_wg_gemm")
    assert n_fp32 == 2 * 9 and not any(k.startswith("conv_wgs_") for k in rows_plain)          # conv3_1 .. conv5_1, both directions
    assert _check_calls(split, calls) == (3, 3)                                                 # conv3_2-4
    assert _launches(rows, "conv_wgs_gemm") == 6 and _launches(rows, "conv_wg_gemm") == n_fp32 - 6
    for m in split.modules():
        d = m.__dict__.get("_wg_frozen")
        if d is not None:
            assert sorted(map(str, (k for k in d if k != "key"))) == (["s0", "s1"] if tuple(m.weight.shape[:2]) == (256, 256) else ["0", "1"])
    print("VGG19 relu5_1, 256 -> 256 on the split route: max |feature difference| %s, max |input gradient difference| %.3e" % (
        ["%.3e" % (a - b).abs().max().item() for a, b in zip(out, out_plain)], (gx - gx_plain).abs().max().item()))


# ---------------------------------------------------------------------------------------------------- capture
def test_captured_forward_and_backward_replays_the_eager_bits(monkeypatch):
    """VGG19's slices from relu3_1 on (every layer of them routed, forward and data gradient), forward + backward in one graph made
    with graphs.py's helper: the replay gives the bits of the eager call, and no split weight transform is issued by the capture or
    the replays -- they were made by the eager call.
    Every pass differentiates with respect to a leaf of its own and returns detached tensors.  A leaf's AccumulateGrad node remembers
    the stream it was made on and lives as long as any output's grad_fn does (FFWMTrainer._drop_autograd_graph): a leaf shared with an
    eager pass on the default stream, whose outputs are still held, would pull that stream into the capture as a forked branch."""
    from ffwm_amd import conv, graphs, nets, ops
    _open_tables(monkeypatch, conv, "both")
    torch.manual_seed(6)
    vgg = nets.VGG19("relu5_1").cuda().eval()
    conv.wg_set_precision(vgg, "bf16x3")
    vgg.slices = vgg.slices[vgg.slices.index("relu3_1"):]
    x = torch.rand(2, 128, 16, 16, device="cuda")

    def fwd_bwd():
        leaf = x.detach().requires_grad_(True)
        out = list(vgg(leaf).values())
        gx, = torch.autograd.grad(_loss(out), leaf)
        return [t.detach() for t in out] + [gx]
    made = []
    real = ops.conv3x3_wg_split_weights
    monkeypatch.setattr(ops, "conv3x3_wg_split_weights", lambda *a, **k: made.append(1) or real(*a, **k))
    want = [t.clone() for t in fwd_bwd()]
    torch.cuda.synchronize()
    routed = sum(1 for m in vgg.modules() if "_wg_frozen" in m.__dict__)
    assert routed == 9 and len(made) == 2 * routed
    graphs.warm_up(fwd_bwd, 2, sync=True)
    g, got = graphs.capture(fwd_bwd)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    assert len(made) == 2 * routed


# ---------------------------------------------------------------------------------------------------- the trainer
def _step_rows(t, batch):
    """Two eager steps, the second one profiled (whatever a trainer or the process sets up once is behind it) -> ({kernel name:
    launches}, {loss name: value}) of the second."""
    from ffwm_amd import _lib
    t.step(batch, batch_increment=0)
    torch.cuda.synchronize()
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        losses = t.step(batch, batch_increment=0)
        torch.cuda.synchronize()
        rows = _lib.prof_collect()
    finally:
        _lib.prof_enable(False)
        _lib.prof_reset()
    return {k: v["launches"] for k, v in rows.items()}, {k: float(v) for k, v in losses.items()}


def test_trainer_step_under_both_precisions():
    """Eager steps at batch 2 per trainer of one seed: made without the argument, with "fp32", with "bf16x3" (WGS_TABLE opened for
    the classes of WG_TABLE: batch 2 is outside the measured ranges)."""
    from ffwm_amd import conv, trainer
    torch.backends.cudnn.benchmark = False
    batch = trainer.synthetic_batch(2, DEV, seed=3)
    rows, vals = {}, {}
    for name, kw in (("default", {}), ("fp32", {"loss_precision": "fp32"})):
        t = trainer.FFWMTrainer(DEV, seed=0, ngf=16, **kw)
        assert t.loss_precision == "fp32"
        rows[name], vals[name] = _step_rows(t, batch)
        del t
    with pytest.MonkeyPatch.context() as mp:
        every = (1, 1 << 30)
        mp.setattr(conv, "WGS_TABLE", {ck: (every, every) for ck in conv.WG_TABLE})
        t = trainer.FFWMTrainer(DEV, seed=0, ngf=16, loss_precision="bf16x3")
        assert t.loss_precision == "bf16x3" and t.wg_weight_bytes > 0
        assert all(conv._wg_precision(m) == "bf16x3" for net in (t.vgg, t.lightCNN) for m in net.modules() if isinstance(m, torch.nn.Conv2d))
        assert all(conv._wg_precision(m) == "fp32" for m in t.netG.modules() if isinstance(m, torch.nn.Conv2d))
        rows["bf16x3"], vals["bf16x3"] = _step_rows(t, batch)
        del t
    for k in sorted(vals["fp32"]):
        print("train step, batch 2, loss %-10s fp32 %.9g   bf16x3 %.9g" % (k, vals["fp32"][k], vals["bf16x3"][k]))
    assert all(math.isfinite(v) for v in vals["bf16x3"].values()), vals["bf16x3"]
    assert rows["bf16x3"].get("conv_wgs_gemm", 0) > 0
    assert rows["bf16x3"]["conv_wgs_gemm"] == rows["bf16x3"]["conv_wgs_in"] == rows["bf16x3"]["conv_wgs_out"]
    assert not any(k.startswith("conv_wgs_") for k in rows["fp32"]) and rows["fp32"].get("conv_wg_gemm", 0) > 0
    assert rows["fp32"] == rows["default"]

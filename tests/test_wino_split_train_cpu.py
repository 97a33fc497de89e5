"""The split batched-GEMM Winograd route of the train step's loss networks (loss_precision="bf16x3") without a GPU: the torch
restatement of the data gradient, its ReLU mask and the relu / mfm epilogues (wino_split_train_cases.split_flow_f32) meets the
per-element bounds with SAFETY = 1, carries the exact family through the data gradient bit for bit, and every mutant misses an
assertion; the routing of conv.py -- wg_set_precision, WGS_TABLE, "fp32" as it was; the trainer's argument; the size formulas and the
argument checks of the new entry points against the library."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import conv_bounds as cb  # noqa: E402
import wino_split_cases as ws  # noqa: E402
import wino_split_train_cases as wt  # noqa: E402

_IDS = dict(ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))


def _check_safety_one(bound, got, reduction):
    rho1, post1 = wt.with_safety_one(bound, reduction)
    saved, bound.post = bound.post, post1
    try:
        bound.check(got, rho=rho1)
    finally:
        bound.post = saved


def _same(a, b):
    """torch.equal with NaN equal to NaN."""
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("kind", cb.FAMILIES)
@pytest.mark.parametrize("shape", wt.DGRAD_SHAPES, **_IDS)
def test_data_gradient_restatement_meets_the_bounds_with_safety_one(shape, kind):
    go, w, y, bounds = wt.split_dgrad_case(shape, kind)
    _check_safety_one(bounds[False], wt.split_flow_f32(go, w, data_gradient=True), shape[4])
    _check_safety_one(bounds[True], wt.split_flow_f32(go, w, data_gradient=True, mask=y), shape[4])


@pytest.mark.parametrize("kind", cb.FAMILIES)
@pytest.mark.parametrize("shape", wt.SHAPES, **_IDS)
def test_epilogue_restatement_meets_the_bounds_with_safety_one(shape, kind):
    x, w, b, bounds = wt.split_forward_case(shape, kind)
    for epi in wt.EPILOGUES:
        got = wt.split_flow_f32(x, w, b, epi)
        _check_safety_one(bounds[epi], got, shape[1])
        if epi in ("none", "bias"):          # the restatement of the inference entry, unchanged
            assert _same(got, ws.split_flow_f32(x, w, b, epi))
    pre = wt.split_flow_f32(x, w, b, "bias")
    h = shape[4] // 2
    assert _same(wt.split_flow_f32(x, w, b, "relu"), torch.relu(pre))
    assert _same(wt.split_flow_f32(x, w, b, "mfm"), torch.maximum(pre[:, :h], pre[:, h:]))


def test_exact_family_through_the_data_gradient():
    go, w, three, full, hh = wt.exact_dgrad_inputs()
    assert w.shape == (ws.EXACT_SHAPE[1], ws.EXACT_SHAPE[4], 3, 3)
    got = wt.split_flow_f32(go, w, data_gradient=True)
    assert torch.equal(got, three.float())
    assert not torch.equal(got, full.float()) and not torch.equal(got, hh.float())
    for mutant in ("not_rotated", "not_transposed"):
        assert not torch.equal(wt.split_flow_f32(go, w, data_gradient=True, mutant=mutant), three.float()), mutant


@pytest.mark.parametrize("mutant", wt.MUTANTS)
def test_every_mutant_misses_the_bound(mutant):
    go, w, y, bounds = wt.mutant_case()
    masked = mutant.startswith("mask")
    bound = bounds[masked]
    kw = dict(data_gradient=True, mask=y if masked else None)
    assert bound.measure(wt.split_flow_f32(go, w, **kw))[0] <= 1.0
    ratio, wrong, _ = bound.measure(wt.split_flow_f32(go, w, mutant=mutant, **kw))
    assert ratio > 1.0 or wrong, (mutant, ratio, wrong)


def test_mask_rule_of_the_restatement():
    """mask <= 0 ? 0 : x -- a NaN in the mask lets the value pass, a masked-out infinity or NaN is a zero."""
    x = torch.tensor([1.0, float("inf"), float("nan"), 3.0, 4.0, 5.0]).view(1, 1, 2, 3).repeat(1, 32, 1, 1)
    m = torch.tensor([float("nan"), 0.0, 0.0, -1.0, 2.0, 0.0]).view(1, 1, 2, 3).repeat(1, 32, 1, 1)
    w = torch.zeros(32, 32, 3, 3)
    w[torch.arange(32), torch.arange(32), 1, 1] = 1.0          # the identity
    want = torch.ops.aten.threshold_backward(x, m, 0)
    assert torch.equal(want[0, 0].flatten(), torch.tensor([1.0, 0.0, 0.0, 0.0, 4.0, 0.0]))
    assert torch.equal(wt.split_flow_f32(x, w, mask=m), want)


# ---------------------------------------------------------------------------------------------------- the routing
# every distinct frozen 3 x 3 / stride-1 shape (B, C, H, W, K) of the train step's loss networks at batch 8 on planes of 32 x 32 and
# below, as tools/wino_gemm_layers.py lists them by running the networks (profiles/wino_gemm_layers.txt): VGG19 on the 128 px and
# 64 px images and on the 40 crops of 32 px, LightCNN-29 on the 128 px image
STEP_SHAPES = [(8, 128, 32, 32, 256), (8, 256, 32, 32, 256), (8, 256, 16, 16, 512), (8, 512, 16, 16, 512), (8, 512, 8, 8, 512),
               (8, 64, 32, 32, 128), (8, 128, 32, 32, 128), (8, 128, 16, 16, 256), (8, 256, 16, 16, 256), (8, 256, 8, 8, 512),
               (8, 512, 4, 4, 512), (40, 128, 8, 8, 256), (40, 256, 8, 8, 256), (40, 256, 4, 4, 512), (40, 512, 4, 4, 512),
               (40, 512, 2, 2, 512), (8, 96, 32, 32, 192), (8, 96, 32, 32, 384), (8, 192, 16, 16, 384), (8, 192, 16, 16, 256)]


def _step_shapes():
    return STEP_SHAPES


def _layer(C, K):
    m = nn.Conv2d(C, K, 3, 1, 1)
    m.weight.requires_grad_(False)
    return m


def test_set_precision_validates_and_stamps():
    from ffwm_amd import conv
    net = nn.Sequential(_layer(8, 8), nn.ReLU(), nn.Sequential(_layer(8, 4)))
    for bad in ("bf16", "fp16", None, 3):
        with pytest.raises(ValueError, match="precision must be"):
            conv.wg_set_precision(net, bad)
    assert conv._wg_precision(net[0]) == "fp32" and conv._wg_precision(None) == "fp32"
    assert conv.wg_set_precision(net, "bf16x3") == 2
    other = nn.Sequential(_layer(8, 8))
    assert [conv._wg_precision(m) for m in (net[0], net[2][0], other[0])] == ["bf16x3", "bf16x3", "fp32"]          # not process-wide
    assert conv.wg_set_precision(net, "fp32") == 2 and conv._wg_precision(net[0]) == "fp32"


def test_fp32_routes_are_unchanged(monkeypatch):
    """Under "fp32" WGS_TABLE is never consulted: with every class of it opened to every T, the routes of every shape of the train step
    are those WG_TABLE alone gives."""
    from ffwm_amd import conv
    every = (1, 1 << 30)
    opened = {ck: (every, every) for ck in list(conv.WG_TABLE) + [(64, 128), (128, 128)]}
    monkeypatch.setattr(conv, "WGS_TABLE", opened)
    for B, C, H, W, K in _step_shapes():
        w = _layer(C, K).weight
        t = B * ((H + 1) // 2) * ((W + 1) // 2)
        fwd, dg = conv.WG_TABLE.get((C, K), (conv._WG_NEVER, conv._WG_NEVER))
        want = tuple("fp32" if r[0] <= t <= r[1] else None for r in (fwd, dg))
        assert tuple(conv.wg_route(t, w, "fp32", d) for d in (0, 1)) == want, (B, C, H, W, K)
        assert all(conv.wg_route(t, w, "bf16x3", d) == ("split" if (C, K) in opened else None) for d in (0, 1))


def test_wgs_table_is_well_formed():
    from ffwm_amd import conv
    assert isinstance(conv.WGS_TABLE, dict)
    measured = {(C, K) for _, C, _, _, K in _step_shapes()}
    tiles = {}
    for B, C, H, W, K in _step_shapes():
        tiles.setdefault((C, K), set()).add(B * ((H + 1) // 2) * ((W + 1) // 2))
    for ck, ranges in conv.WGS_TABLE.items():
        assert ck in measured, ck                                          # a class of the train step
        assert len(ranges) == 2
        for lo, hi in ranges:
            assert isinstance(lo, int) and isinstance(hi, int)
            assert (lo, hi) == conv._WG_NEVER or (lo <= hi and lo in tiles[ck] and hi in tiles[ck]), (ck, lo, hi)          # ends: measured shapes
        assert ranges[0] != conv._WG_NEVER, ck                             # a data gradient is routed only behind a routed forward


def test_a_layer_outside_wgs_table_keeps_its_route(monkeypatch):
    from ffwm_amd import conv
    monkeypatch.setattr(conv, "WGS_TABLE", {(256, 256): ((512, 512), conv._WG_NEVER)})
    for B, C, H, W, K in _step_shapes():
        w = _layer(C, K).weight
        t = B * ((H + 1) // 2) * ((W + 1) // 2)
        for d in (0, 1):
            if (C, K, t, d) == (256, 256, 512, 0):
                assert conv.wg_route(t, w, "bf16x3", d) == "split"
            else:
                assert conv.wg_route(t, w, "bf16x3", d) == conv.wg_route(t, w, "fp32", d), (B, C, H, W, K, d)
    # wg_ok on the CPU: never (the route is a HIP kernel), whatever the stamp says
    m = _layer(256, 256)
    conv.wg_set_precision(nn.Sequential(m), "bf16x3")
    assert not conv.wg_ok(torch.zeros(8, 256, 16, 16), m.weight, m)


def test_trainer_refuses_bf16x3_on_the_cpu():
    from ffwm_amd.trainer import FFWMTrainer
    with pytest.raises(ValueError, match="bf16x3"):
        FFWMTrainer("cpu", ngf=4, loss_precision="bf16x3")
    with pytest.raises(ValueError, match="loss_precision must be"):
        FFWMTrainer("cpu", ngf=4, loss_precision="bf16")
    with pytest.raises(ValueError, match="loss_precision must be"):
        FFWMTrainer("cpu", ngf=4, loss_precision=None)


# ---------------------------------------------------------------------------------------------------- the library
@pytest.fixture(scope="module")
def hiplib():
    from ffwm_amd import build, _lib
    build.build()
    return _lib.load()


def test_symbols_sizes_and_argument_errors(hiplib):
    from ffwm_amd import _lib
    for name in ("ffwm_conv3x3_wg_split_weights_dgrad", "ffwm_conv3x3_wg_split_apply"):
        assert hasattr(hiplib, name) and name in _lib.EXPORTS, name
    assert hiplib.ffwm_abi_version() == 5
    # the data gradient of a layer (C, K): U with C rows over K rounded up to 32; its call is a convolution K -> C
    for B, C, H, W, K in wt.DGRAD_SHAPES + [(8, 512, 16, 16, 512), (16, 96, 32, 32, 384)]:
        assert hiplib.ffwm_conv3x3_wg_split_weights_bytes(K, C) == wt.weights_bytes(K, C)
        assert hiplib.ffwm_conv3x3_wg_split_weights_bytes(C, K) == wt.weights_bytes(C, K)
        assert hiplib.ffwm_conv3x3_wg_split_workspace_bytes(B, C, H, W, K) == wt.workspace_bytes(B, C, H, W, K)
        assert hiplib.ffwm_conv3x3_wg_split_workspace_bytes(B, K, H, W, C) == wt.workspace_bytes(B, K, H, W, C)
    assert wt.weights_bytes(70, 19) == 16 * 32 * 70 * 4 and wt.weights_bytes(19, 70) == 16 * 96 * 19 * 4

    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value // 16 * 16 + 16
    run, err = hiplib.ffwm_conv3x3_wg_split_apply, hiplib.ffwm_last_error
    assert run(None, None, None, None, None, 1, 8, 4, 4, 8, 0, None, 0, 0, None) == -1 and b"NULL" in err()
    assert run(p, p, None, p, None, 1, 8, 4, 4, 8, 0, None, 0, 0, None) == -1 and b"NULL" in err()
    assert run(p, p, None, p, p, 1, 8, 4, 0, 8, 0, None, 0, 0, None) == -1 and b"positive" in err()
    assert run(p, p, p, p, p, 1, 8, 4, 4, 8, 4, None, 0, 0, None) == -1 and b"epilogue" in err()
    assert run(p, p, p, p, p, 1, 8, 4, 4, 8, -1, None, 0, 0, None) == -1 and b"epilogue" in err()
    assert run(p, p, p, p, p, 1, 8, 4, 4, 8, 0x100, None, 0, 0, None) == -1 and b"epilogue" in err()      # no hidden bits
    for epi in (1, 2, 3):
        assert run(p, p, None, p, p, 1, 8, 4, 4, 8, epi, None, 0, 0, None) == -1 and b"bias" in err()
    assert run(p, p, p, p, p, 1, 8, 4, 4, 7, 3, None, 0, 0, None) == -1 and b"even" in err()
    assert run(p, p, None, p, p, 1, 8, 4, 4, 8, 0, None, 32, 0, None) == -1 and b"tile" in err()
    assert run(p, p + 4, None, p, p, 1, 8, 4, 4, 8, 0, None, 0, 0, None) == -1 and b"aligned" in err()
    assert run(p, p, None, p, p + 8, 1, 8, 4, 4, 8, 0, p, 0, 0, None) == -1 and b"aligned" in err()
    assert run(p, p, None, p, p, 1, 8, 4, 4, 8, 0, None, 0, 1, None) == -2 and b"float32" in err()
    assert run(p, p, None, p, p, 1 << 12, 1 << 10, 1 << 5, 1 << 5, 8, 0, None, 0, 0, None) == -3
    wts = hiplib.ffwm_conv3x3_wg_split_weights_dgrad
    assert wts(None, p, 8, 8, 0, None) == -1 and b"NULL" in err()
    assert wts(p, p, 0, 8, 0, None) == -1 and wts(p, p, 8, 0, 0, None) == -1
    assert wts(p, p + 4, 8, 8, 0, None) == -1 and b"aligned" in err()
    assert wts(p, p, 8, 8, 1, None) == -2
    assert wts(p, p, 1 << 16, 1 << 16, 0, None) == -3
    # the inference entry keeps refusing what only the new one takes
    assert hiplib.ffwm_conv3x3_wg_split_forward(p, p, p, p, p, 1, 8, 4, 4, 8, 3, 0.2, 0, 0, None) == -1 and b"epilogue" in err()

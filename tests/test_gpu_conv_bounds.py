"""The convolution kernels against the per-element yardstick of tests/conv_bounds.py: every element within rho mag of ATen's float64
result (rho derived per kernel from its accumulation structure, mag the element's own sum of |products| -- or the Winograd patch
magnitude), non-finite elements exactly where the reference has them, and small-integer cases bit for bit.  A matrix of entry point x
kernel path x input family; every path is asserted to have run through its profiler scope, every option is restored in `finally`.
`iid` and `integers` run at every shape, the other families at the shapes marked `all`.  Run with ``-m gpu`` on the MI355X."""
import contextlib

import pytest
import torch

import conv_bounds as cb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BASIC = ("iid", "integers")


def _kinds(every):
    return cb.FAMILIES if every else BASIC


@contextlib.contextmanager
def _scoped(options=None):
    """Set `options`, profile what runs inside, put the options back; yields the dict the scopes' launch counts are collected into."""
    from ffwm_amd import _lib
    rows, prev = {}, {}
    try:
        for k, v in (options or {}).items():
            prev[k] = _lib.set_option(k, v)
        _lib.prof_reset()
        _lib.prof_enable(True)
        yield rows
        torch.cuda.synchronize()
        rows.update({k: v["launches"] for k, v in _lib.prof_collect().items()})
    finally:
        _lib.prof_enable(False)
        for k, v in prev.items():
            _lib.set_option(k, v)


def _ran(rows, *scopes):
    for s in scopes:
        assert rows.get(s, 0) >= 1, (s, rows)


def _not_ran(rows, *scopes):
    for s in scopes:
        assert s not in rows, (s, rows)


def _cases(table):
    return [pytest.param(name, kind, id="%s-%s" % (name, kind)) for name, spec in table.items() for kind in _kinds(spec[-1])]


# ------------------------------------------------------------------------------------------------ conv_fwd.hip: modes 0-3
FWD_SCOPE = ("conv_fwd_mfma", "conv_fwd_mfma_transposed", "conv_dgrad_mfma_3x3s2", "conv_dgrad_mfma_3x3s1")
# name: (B, C of the tensor read, H, W, K written, kernel, stride, pad, mode, expect a split launch, all families)
FWD = {
    "tiny_s2": (2, 3, 16, 16, 8, 3, 2, 1, 0, None, True),
    "conv6": (6, 512, 4, 4, 1024, 3, 2, 1, 0, True, False),
    "conv6_1": (6, 1024, 2, 2, 1024, 3, 1, 1, 0, True, False),
    "ragged": (3, 70, 9, 11, 130, 3, 1, 1, 0, None, True),
    "enc4x4": (2, 64, 32, 32, 128, 4, 2, 1, 0, None, False),
    "deconv5": (6, 1024, 2, 2, 512, 4, 2, 1, 1, True, False),
    "deconv_ragged": (2, 5, 7, 9, 3, 4, 2, 1, 1, None, True),
    "deconv_25": (2, 24, 25, 25, 100, 4, 2, 1, 1, None, False),
    # mode 2: d(input) of Conv2d(K, C, 3, 2, 1) -- grad_output [B, C, H, W] -> [B, K, 2H, 2W]
    "m2_conv6": (8, 1024, 2, 2, 512, 3, 2, 1, 2, True, False),
    "m2_conv5": (6, 512, 4, 4, 512, 3, 2, 1, 2, True, True),
    "m2_ragged": (3, 130, 5, 6, 70, 3, 2, 1, 2, None, True),
    "m2_16": (2, 96, 16, 16, 64, 3, 2, 1, 2, None, False),
    # mode 3: d(input) of Conv2d(K, C, 3, 1, 1) -- FlowNet's conv6_1 / conv5_1 / inter_conv5 / inter_conv4
    "m3_conv6_1": (8, 1024, 2, 2, 1024, 3, 1, 1, 3, True, False),
    "m3_conv5_1": (6, 512, 4, 4, 512, 3, 1, 1, 3, True, False),
    "m3_inter5": (8, 512, 4, 4, 1026, 3, 1, 1, 3, True, True),
    "m3_inter4": (6, 256, 8, 8, 770, 3, 1, 1, 3, None, False),
    "m3_ragged": (3, 130, 9, 11, 70, 3, 1, 1, 3, None, True),
}


def _fwd_operands(name, kind):
    B, C, H, W, K, k, stride, pad, mode, _, _ = FWD[name]
    seed = sum(FWD[name][:5])
    x = cb.activations(kind, (B, C, H, W), seed)
    w, b = cb.weights(kind, (K, C, k, k) if mode == 0 else (C, K, k, k), seed + 1, out_dim=0 if mode == 0 else 1)
    return x, w, (b if mode < 2 else None)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name,kind", _cases(FWD))
def test_conv_mfma_per_element(name, kind, split):
    from ffwm_amd import _lib, flownet_eval
    B, C, H, W, K, k, stride, pad, mode, want_split, _ = FWD[name]
    x, w, b = _fwd_operands(name, kind)
    exact = kind == "integers"
    act = flownet_eval.NONE if mode >= 2 else flownet_eval.LRELU
    slope = 0.0 if exact else 0.2
    bound = cb.forward_bound(x, w, b, stride, pad, mode, act, slope, None, exact=exact)
    need = _lib.load().ffwm_conv2d_forward_workspace(B, C, H, W, K, k, stride, pad, mode)          # splitk slots of the output's size
    splitk = max(need // (4 * bound.ref.numel()), 1) if split else 1
    bound.rho = cb.rho_conv_fwd(C, 4 if mode in (1, 2) else k * k, splitk)
    bound.what = "conv_fwd mode %d %s %s split %d" % (mode, name, kind, splitk)
    with _scoped() as rows:
        y = flownet_eval.conv_mfma(x.to(DEV), w.to(DEV), None if b is None else b.to(DEV), stride, pad, mode, act, slope, split=split)
    _ran(rows, FWD_SCOPE[mode])
    if split and want_split:
        assert splitk > 1
        _ran(rows, "conv_fwd_split_reduce")
    if not split:
        _not_ran(rows, "conv_fwd_split_reduce")
    bound.check(y)


@pytest.mark.parametrize("variant", [1, 2, 3, 4])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", ["iid", "integers", "out_scales", "spike"])
def test_conv_mfma_tile_variants_and_destinations(kind, mode, variant):
    """Every workgroup tile shape on ragged channel tiles and ragged pixel blocks, written into a channel slice of a wider buffer and
    into a second destination; the neighbouring channels of both buffers stay untouched."""
    from ffwm_amd import flownet_eval
    B, C, H, W, K = 2, 20, (37 if mode in (0, 3) else 13), (37 if mode in (0, 3) else 14), 100
    k = 4 if mode == 1 else 3
    stride = 2 if mode in (1, 2) else 1
    x = cb.activations(kind, (B, C, H, W), 40 + mode)
    w, b = cb.weights(kind, (K, C, k, k) if mode == 0 else (C, K, k, k), 41 + mode, out_dim=0 if mode == 0 else 1)
    exact = kind == "integers"
    act, slope = (flownet_eval.LRELU, 0.0 if exact else 0.2)
    bound = cb.forward_bound(x, w, b, stride, 1, mode, act, slope, cb.rho_conv_fwd(C, 4 if mode in (1, 2) else 9), exact=exact,
                             what="conv_fwd mode %d variant %d %s" % (mode, variant, kind))
    Ho, Wo = bound.ref.shape[2:]
    buf = torch.full((B, K + 5, Ho, Wo), 7.0, device=DEV)
    buf2 = torch.full((B, K + 3, Ho, Wo), 9.0, device=DEV)
    with _scoped({"conv_tile_variant": variant}) as rows:
        flownet_eval.conv_mfma(x.to(DEV), w.to(DEV), b.to(DEV), stride, 1, mode, act, slope, dst=buf[:, 2:2 + K], dst2=buf2[:, 3:], split=False)
    _ran(rows, FWD_SCOPE[mode])
    bound.check(buf[:, 2:2 + K])
    assert torch.equal(buf2[:, 3:], buf[:, 2:2 + K])
    assert bool((buf[:, :2] == 7).all()) and bool((buf[:, 2 + K:] == 7).all()) and bool((buf2[:, :3] == 9).all())


@pytest.mark.parametrize("name", ["conv6", "deconv5", "m2_conv5", "m3_inter5"])
def test_conv_mfma_split_launch_into_destinations(name):
    """A split launch (workspace slots + the fixed-order reduce pass) with bias and activation, into a channel slice + a second buffer."""
    from ffwm_amd import flownet_eval
    B, C, H, W, K, k, stride, pad, mode, _, _ = FWD[name]
    x, w, _ = _fwd_operands(name, "integers")
    _, b = cb.weights("integers", w.shape, 5, out_dim=0 if mode == 0 else 1)
    bound = cb.forward_bound(x, w, b, stride, pad, mode, flownet_eval.LRELU, 0.0, cb.rho_conv_fwd(C, 9, 64), exact=True, what="split dst " + name)
    Ho, Wo = bound.ref.shape[2:]
    buf = torch.full((B, K + 4, Ho, Wo), 7.0, device=DEV)
    buf2 = torch.full((B, K + 4, Ho, Wo), 9.0, device=DEV)
    with _scoped() as rows:
        flownet_eval.conv_mfma(x.to(DEV), w.to(DEV), b.to(DEV), stride, pad, mode, flownet_eval.LRELU, 0.0, dst=buf[:, 4:], dst2=buf2[:, :K])
    _ran(rows, FWD_SCOPE[mode], "conv_fwd_split_reduce")
    bound.check(buf[:, 4:])
    assert torch.equal(buf2[:, :K], buf[:, 4:]) and bool((buf[:, :4] == 7).all()) and bool((buf2[:, K:] == 9).all())


# ------------------------------------------------------------------------------------------------ conv_winograd.hip
# name: (B, C, H, W, K, all families)
WINO = {
    "tiny": (1, 8, 4, 4, 64, False),
    "odd": (2, 19, 7, 9, 70, True),
    "ragged": (3, 33, 17, 30, 130, False),
    "res195": (2, 195, 64, 64, 195, True),
    "wide128": (2, 96, 128, 128, 48, False),
    "tail1": (1, 66, 8, 12, 65, False),
    "tail3": (2, 68, 9, 16, 131, True),
    "gather": (2, 40, 15, 16, 64, False),
    "head3": (2, 70, 32, 32, 3, True),
    "head1": (1, 33, 8, 12, 1, False),
}


def _wino_ran(rows, data_gradient, K_out, W):
    """The thin kernel takes 1-4 output channels past a multiple of 64 (or an image head of <= 4) when the width is a multiple of 4."""
    thin = (K_out > 64 or K_out <= 4) and 1 <= K_out % 64 <= 4 and W % 4 == 0
    if thin:
        _ran(rows, "conv3x3_thin_tail")
    else:
        _not_ran(rows, "conv3x3_thin_tail")
    if K_out > 4 or not thin:
        assert any(k.startswith("conv_winograd_dgrad" if data_gradient else "conv_winograd_fwd") for k in rows), rows


# (conv_wino_raw = 0, the gather variant: iid and integers everywhere, every family at one shape)
@pytest.mark.parametrize("name,kind,raw", [pytest.param(n, k, r, id="%s-%s-raw%d" % (n, k, r)) for n, s in WINO.items() for k in _kinds(s[-1])
                                           for r in (1, 0) if r == 1 or k in BASIC or n == "odd"])
def test_winograd_forward_and_data_gradient_per_element(name, kind, raw):
    from ffwm_amd import ops
    B, C, H, W, K, every = WINO[name]
    exact = kind == "integers"
    seed = B + C + H + W + K
    x = cb.activations(kind, (B, C, H, W), seed)
    w, b = cb.weights(kind, (K, C, 3, 3), seed + 1)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    slope = 0.0 if exact else 0.2
    fb = cb.forward_bound(x, w, b, 1, 1, 0, 1, slope, cb.rho_winograd(C), winograd=True, exact=exact, what="winograd fwd %s %s raw %d" % (name, kind, raw))
    with _scoped({"conv_wino_raw": raw}) as rows:
        y = ops.conv3x3_winograd(xd, wd, bd, act=1, slope=slope)
    _wino_ran(rows, False, K, W)
    fb.check(y)
    go = cb.grad_outputs(kind, (B, K, H, W), seed + 2)
    db = cb.forward_bound(go, w, None, 1, 1, 3, rho=cb.rho_winograd(K), winograd=True, exact=exact, what="winograd dgrad %s %s raw %d" % (name, kind, raw))
    with _scoped({"conv_wino_raw": raw}) as rows:
        dx = ops.conv3x3_winograd(go.to(DEV), wd, None, data_gradient=True)
    _wino_ran(rows, True, C, W)
    db.check(dx)


WINO_SPLIT = {"split2": (8, 256, 32, 32, 256, 2, False), "split4": (8, 512, 16, 16, 512, 4, False), "split2_tail": (2, 256, 32, 32, 195, 2, True)}


@pytest.mark.parametrize("split", [1, 0])
@pytest.mark.parametrize("name,kind", [pytest.param(n, k, id="%s-%s" % (n, k)) for n, s in WINO_SPLIT.items() for k in _kinds(s[-1])])
def test_winograd_split_reduction_per_element(name, kind, split):
    """Calls with few (64 tiles, 64 channels) pairs cut the input-channel reduction over 2 / 4 workgroups whose partial outputs meet
    by float atomics in the output the library zero-fills; conv_wino_split 0 keeps one piece."""
    from ffwm_amd import ops
    B, C, H, W, K, want, _ = WINO_SPLIT[name]
    assert ops.conv3x3_winograd_splits(B, C, H, W, K, 0) == want
    exact = kind == "integers"
    x = cb.activations(kind, (B, C, H, W), 70, small=True)
    w, b = cb.weights(kind, (K, C, 3, 3), 71, small=True)
    pieces = want if split else 1
    fb = cb.forward_bound(x, w, b, 1, 1, 0, None, 0.0, cb.rho_winograd(C, pieces), winograd=True, exact=exact, what="winograd fwd %s %s split %d" % (name, kind, split))
    out = torch.full((B, K, H, W), 7.0, device=DEV)
    with _scoped({"conv_wino_split": split}) as rows:
        ops.conv3x3_winograd(x.to(DEV), w.to(DEV), b.to(DEV), out=out)
    _ran(rows, "conv_winograd_fwd_split" if split else "conv_winograd_fwd")
    fb.check(out)
    go = cb.grad_outputs(kind, (B, K, H, W), 72, small=True)
    dsplits = ops.conv3x3_winograd_splits(B, K, H, W, C, 0) if split else 1
    db = cb.forward_bound(go, w, None, 1, 1, 3, rho=cb.rho_winograd(K, dsplits), winograd=True, exact=exact, what="winograd dgrad %s %s split %d" % (name, kind, split))
    with _scoped({"conv_wino_split": split}) as rows:
        dx = ops.conv3x3_winograd(go.to(DEV), w.to(DEV), None, data_gradient=True)
    assert any(k.startswith("conv_winograd_dgrad") for k in rows), rows
    db.check(dx)


@pytest.mark.parametrize("kind", ["iid", "integers", "in_scales", "spike"])
@pytest.mark.parametrize("shape", [(2, 64, 32, 32, 64), (2, 195, 64, 64, 195), (3, 72, 16, 16, 130)])
def test_winograd_wave_specialised_and_prepared_weights_per_element(shape, kind):
    """conv_wino_ws = 1, a layer-owned cache of the transformed weights (`frozen`: the second call reuses it) and transforms prepared
    by conv3x3_winograd_weights_multi (`pre`), forward and data gradient."""
    from ffwm_amd import ops
    B, C, H, W, K = shape
    exact = kind == "integers"
    x = cb.activations(kind, (B, C, H, W), 80)
    w, b = cb.weights(kind, (K, C, 3, 3), 81)
    go = cb.grad_outputs(kind, (B, K, H, W), 82)
    xd, wd, bd, god = x.to(DEV), w.to(DEV), b.to(DEV), go.to(DEV)
    fb = cb.forward_bound(x, w, b, 1, 1, 0, None, 0.0, cb.rho_winograd(C), winograd=True, exact=exact, what="winograd fwd %s %s" % (shape, kind))
    db = cb.forward_bound(go, w, None, 1, 1, 3, rho=cb.rho_winograd(K), winograd=True, exact=exact, what="winograd dgrad %s %s" % (shape, kind))
    with _scoped({"conv_wino_ws": 1}) as rows:
        y, dx = ops.conv3x3_winograd(xd, wd, bd), ops.conv3x3_winograd(god, wd, None, data_gradient=True)
    _ran(rows, "conv_winograd_fwd", "conv_winograd_dgrad")
    fb.check(y, fb.what + " ws")
    db.check(dx, db.what + " ws")
    cache = {}
    for i in range(2):
        with _scoped() as rows:
            y, dx = ops.conv3x3_winograd(xd, wd, bd, frozen=cache), ops.conv3x3_winograd(god, wd, None, data_gradient=True, frozen=cache)
        assert ("conv_winograd_weights" in rows) == (i == 0), rows
        fb.check(y, fb.what + " frozen %d" % i)
        db.check(dx, db.what + " frozen %d" % i)
    pre = dict(zip(((0, W % 4 == 0), (1, W % 4 == 0)), ops.conv3x3_winograd_weights_multi([(wd, False, W % 4 == 0), (wd, True, W % 4 == 0)])))
    with _scoped() as rows:
        y, dx = ops.conv3x3_winograd(xd, wd, bd, pre=pre), ops.conv3x3_winograd(god, wd, None, data_gradient=True, pre=pre)
    _not_ran(rows, "conv_winograd_weights")
    fb.check(y, fb.what + " pre")
    db.check(dx, db.what + " pre")


# ------------------------------------------------------------------------------------------------ conv_wgrad.hip / conv_wgrad_wino.hip
# name: (B, C, K, H, W, scopes that must run with the direct kernel, all families)
WG3 = {
    "dres2": (2, 195, 195, 16, 64, ("conv3x3_wgrad", "conv3x3_wgrad_packed"), True),
    "strips": (1, 64, 64, 9, 128, ("conv3x3_wgrad",), False),
    "thin_c": (3, 7, 70, 5, 64, ("conv3x3_wgrad",), False),
    "row_chunks": (2, 128, 33, 40, 64, ("conv3x3_wgrad",), False),
    "both_thin": (1, 67, 130, 6, 64, ("conv3x3_wgrad", "conv3x3_wgrad_packed"), True),
    "swapped": (1, 64, 193, 7, 64, ("conv3x3_wgrad", "conv3x3_wgrad_packed", "conv_bias_rows"), False),
    "rgb_in": (2, 3, 195, 6, 128, ("conv3x3_wgrad_packed", "conv_bias_rows"), True),
    "rgb_out": (2, 195, 3, 6, 64, ("conv3x3_wgrad_packed", "conv_bias_rows"), False),
    "thin_both": (1, 2, 1, 5, 64, ("conv3x3_wgrad_packed",), False),
}


@pytest.mark.parametrize("name,kind", _cases(WG3))
def test_conv3x3_wgrad_direct_per_element(name, kind):
    """The direct, packed and swapped-packed variants (conv_wgrad_wino = 2: never the Winograd-domain kernel), the fused bias
    gradient, and a second call that accumulates (+=) into the first result."""
    from ffwm_amd import ops
    B, C, K, H, W, scopes, _ = WG3[name]
    exact = kind == "integers"
    x = cb.activations(kind, (B, C, H, W), 90 + C)
    go = cb.grad_outputs(kind, (B, K, H, W), 91 + K)
    wb, bb = cb.wgrad_bounds(x, go, 3, 1, 1, rho=cb.rho_wgrad3x3(B, C, K, H, W), exact=exact, what="conv3x3_wgrad %s %s" % (name, kind))
    xd, god = x.to(DEV), go.to(DEV)
    gw, gb = torch.zeros(K, C, 3, 3, device=DEV), torch.zeros(K, device=DEV)
    with _scoped({"conv_wgrad_wino": 2}) as rows:
        ops.conv3x3_wgrad(xd, god, gw, gb)
    _ran(rows, *scopes)
    _not_ran(rows, "conv3x3_wgrad_winograd")
    wb.check(gw)
    bb.check(gb)
    if kind not in ("nonfinite",):
        first = gw.clone()
        wb2, _ = cb.wgrad_bounds(x, go, 3, 1, 1, rho=cb.rho_wgrad3x3(B, C, K, H, W, True), exact=exact, what=wb.what + " +=", init=first)
        with _scoped({"conv_wgrad_wino": 2}):
            ops.conv3x3_wgrad(xd, god, gw)
        wb2.check(gw)


# name: (B, C, K, H, W, slices expected > 1, all families)
WGW = {
    "split16": (2, 64, 64, 64, 64, True, True),
    "unsplit": (1, 64, 64, 8, 64, False, False),
    "ragged": (3, 70, 131, 32, 64, True, True),
    "two_rows": (8, 64, 64, 2, 128, True, False),
    "res195": (2, 195, 195, 64, 64, True, False),
}


@pytest.mark.parametrize("name,kind", _cases(WGW))
def test_conv3x3_wgrad_winograd_domain_per_element(name, kind):
    """conv_wgrad_wino = 1: the full 64-channel tiles on the Winograd-domain kernel (remainders on the packed direct kernel), with
    the bias gradient; then accumulating into the first result."""
    from ffwm_amd import ops
    B, C, K, H, W, sliced, _ = WGW[name]
    assert (cb.wgrad_wino_structure(B, C, K, H, W)[1] > 1) == sliced
    exact = kind == "integers"
    x = cb.activations(kind, (B, C, H, W), 95 + C, small=True)
    go = cb.grad_outputs(kind, (B, K, H, W), 96 + K, small=True)
    rho = max(cb.rho_wgrad_wino(B, C, K, H, W), cb.rho_wgrad3x3(B, C, K, H, W))
    wb, bb = cb.wgrad_bounds(x, go, 3, 1, 1, rho=rho, winograd=True, exact=exact,
                             what="conv3x3_wgrad winograd %s %s" % (name, kind))
    xd, god = x.to(DEV), go.to(DEV)
    gw, gb = torch.zeros(K, C, 3, 3, device=DEV), torch.zeros(K, device=DEV)
    with _scoped({"conv_wgrad_wino": 1}) as rows:
        ops.conv3x3_wgrad(xd, god, gw, gb)
    assert rows.get("conv3x3_wgrad_winograd", 0) == 1 and "conv3x3_wgrad" not in rows, rows
    wb.check(gw)
    bb.check(gb)
    if kind != "nonfinite":
        wb2, _ = cb.wgrad_bounds(x, go, 3, 1, 1, rho=rho + cb.SAFETY * 16 * cb.U32, winograd=True, exact=exact, what=wb.what + " +=", init=gw.clone())
        with _scoped({"conv_wgrad_wino": 1}):
            ops.conv3x3_wgrad(xd, god, gw)
        wb2.check(gw)


# ------------------------------------------------------------------------------------------------ conv_bwd.hip
# name: (B, C, H, W, K, kernel, stride, pad, transposed, all families)
WGB = {
    "tiny_s2": (2, 3, 16, 16, 8, 3, 2, 1, False, True),
    "conv6": (8, 512, 4, 4, 1024, 3, 2, 1, False, False),
    "inter5": (8, 1026, 4, 4, 512, 3, 1, 1, False, True),
    "ragged": (3, 70, 10, 12, 130, 3, 1, 1, False, True),
    "enc4x4": (2, 64, 32, 32, 128, 4, 2, 1, False, False),
    "deconv5": (8, 1024, 2, 2, 512, 4, 2, 1, True, False),
    "deconv_ragged": (2, 5, 6, 10, 3, 4, 2, 1, True, True),
    "flow_up": (8, 2, 16, 16, 2, 4, 2, 1, True, False),
    "head2": (8, 16, 128, 128, 2, 3, 1, 1, False, False),
    "att64": (2, 64, 64, 64, 128, 3, 1, 1, False, False),
    "short195": (2, 195, 64, 64, 195, 1, 1, 0, False, False),
    "ragged_1x1": (3, 70, 10, 12, 130, 1, 1, 0, False, True),
}


def _wgb_operands(name, kind):
    B, C, H, W, K, k, stride, pad, transposed, _ = WGB[name]
    Ho, Wo = (2 * H, 2 * W) if transposed else ((H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1)
    x = cb.activations(kind, (B, C, H, W), 60 + C)
    go = cb.grad_outputs(kind, (B, K, Ho, Wo), 61 + K)
    return x, go


# (conv_wgrad_unsliced = 1: iid and integers everywhere, every family at one shape)
@pytest.mark.parametrize("name,kind,unsliced", [pytest.param(n, k, u, id="%s-%s-unsliced%d" % (n, k, u)) for n, s in WGB.items() for k in _kinds(s[-1])
                                                for u in (0, 1) if u == 0 or k in BASIC or n == "ragged"])
def test_conv2d_wgrad_tiled_per_element(name, kind, unsliced):
    from ffwm_amd import ops
    B, C, H, W, K, k, stride, pad, transposed, _ = WGB[name]
    x, go = _wgb_operands(name, kind)
    exact = kind == "integers"
    rows_t, gath = (x, go) if transposed else (go, x)
    P, N = rows_t.shape[2] * rows_t.shape[3], gath.shape[1] * k * k
    rho = cb.rho_wgrad_tiled(B, rows_t.shape[1], P, N, bool(unsliced))
    wb, bb = cb.wgrad_bounds(x, go, k, stride, pad, transposed, rho=rho, exact=exact, what="conv2d_wgrad_tiled %s %s unsliced %d" % (name, kind, unsliced))
    with _scoped({"conv_wgrad_unsliced": unsliced}) as rows:
        gw, gb = ops.conv2d_wgrad_tiled(rows_t.to(DEV), gath.to(DEV), k, stride, pad, want_bias=not transposed)
    _ran(rows, "conv_wgrad_mfma_tiled")
    wb.check(gw)
    if not transposed:
        bb.check(gb)


@pytest.mark.parametrize("name,kind", _cases(WGB))
def test_conv2d_wgrad_generic_per_element(name, kind):
    from ffwm_amd import ops
    B, C, H, W, K, k, stride, pad, transposed, _ = WGB[name]
    x, go = _wgb_operands(name, kind)
    exact = kind == "integers"
    rows_t, gath = (x, go) if transposed else (go, x)
    P, N = rows_t.shape[2] * rows_t.shape[3], gath.shape[1] * k * k
    wb, _ = cb.wgrad_bounds(x, go, k, stride, pad, transposed, rho=cb.rho_wgrad_generic(B, rows_t.shape[1], P, N), exact=exact,
                            what="conv2d_wgrad generic %s %s" % (name, kind))
    with _scoped() as rows:
        gw = ops.conv2d_wgrad(rows_t.to(DEV), gath.to(DEV), k, stride, pad)
    _ran(rows, "conv_wgrad_mfma_generic")
    wb.check(gw)


# ------------------------------------------------------------------------------------------------ the thin kernels of flownet_ops.hip
# (the last two resolve to 16 pixels per block -- the second ends in a partial tile --, the others to 4 or 64: flow_head_tile as
# tests/small_kernel_bounds.py restates it)
FLOW_HEADS = [(8, 1024, 2, 2), (8, 256, 8, 8), (3, 70, 9, 11), (8, 32, 64, 64), (2, 16, 128, 128), (6, 128, 16, 16), (4, 70, 19, 23)]


@pytest.mark.parametrize("shape,kind", [pytest.param(s, k, id="%dx%dx%dx%d-%s" % (s + (k,))) for s in FLOW_HEADS
                                        for k in _kinds(s in ((3, 70, 9, 11), (8, 32, 64, 64), (4, 70, 19, 23)))])
def test_flow_head_per_element(shape, kind):
    """Conv2d(C, 2, 3, 1, 1) + bias + tanh in one launch.  Integers: the pre-activation is exact, so the result is within the 4 ulps
    of tanhf alone (rho = 0)."""
    from ffwm_amd import flownet_eval
    B, C, H, W = shape
    x = cb.activations(kind, shape, 20 + C)
    w, b = cb.weights(kind, (2, C, 3, 3), 21 + C)
    rho = 0.0 if kind == "integers" else cb.rho_any_order(C * 9)
    bound = cb.forward_bound(x, w, b, 1, 1, 0, "tanh", 0.0, rho, what="flow_head %s %s" % (shape, kind))
    if kind == "integers":
        cb.require_exact(bound.mag)
    with _scoped() as rows:
        y = flownet_eval.flow_head(x.to(DEV), w.to(DEV), b.to(DEV))
    _ran(rows, "flownet_flow_head")
    bound.check(y)


@pytest.mark.parametrize("kind", cb.FAMILIES)
@pytest.mark.parametrize("shape", [(8, 2, 2), (8, 16, 16), (3, 7, 9), (8, 64, 64)])
def test_flow_up_per_element(shape, kind):
    """ConvTranspose2d(2, 2, 4, 2, 1) + bias written into the last two channels of a concatenation buffer."""
    from ffwm_amd import flownet_eval
    B, H, W = shape
    x = cb.activations(kind, (B, 2, H, W), 30 + H)
    w, b = cb.weights(kind, (2, 2, 4, 4), 31 + H, out_dim=1)
    exact = kind == "integers"
    bound = cb.forward_bound(x, w, b, 2, 1, 1, None, 0.0, cb.rho_any_order(2 * 4), exact=exact, what="flow_up %s %s" % (shape, kind))
    buf = torch.full((B, 7, 2 * H, 2 * W), 7.0, device=DEV)
    with _scoped() as rows:
        flownet_eval.flow_up(x.to(DEV), w.to(DEV), b.to(DEV), buf[:, 5:])
    _ran(rows, "flownet_flow_up")
    bound.check(buf[:, 5:])
    assert bool((buf[:, :5] == 7).all())


@pytest.mark.parametrize("kind", cb.FAMILIES)
@pytest.mark.parametrize("shape", [(2, 6, 64, 64, 64), (1, 18, 64, 128, 16), (2, 5, 7, 9, 8)])
def test_conv_thin_per_element(shape, kind):
    """Conv2d(C <= 18, K, 3, 1, 1) + bias + LeakyReLU on the direct thin-channel kernel (FlowNet's conv0 / inter_conv0)."""
    from ffwm_amd import flownet_eval
    B, C, H, W, K = shape
    x = cb.activations(kind, (B, C, H, W), 10 + C)
    w, b = cb.weights(kind, (K, C, 3, 3), 11 + C)
    exact = kind == "integers"
    slope = 0.0 if exact else 0.2
    bound = cb.forward_bound(x, w, b, 1, 1, 0, 1, slope, cb.rho_any_order(C * 9), exact=exact, what="conv_thin %s %s" % (shape, kind))
    with _scoped() as rows:
        y = flownet_eval.conv_thin(x.to(DEV), flownet_eval.thin_weights(w).to(DEV), b.to(DEV), flownet_eval.LRELU, slope)
    _ran(rows, "flownet_conv_thin")
    bound.check(y)

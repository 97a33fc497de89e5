"""The one-pass kernels against the yardsticks of tests/small_kernel_bounds.py: mfm and bias + ReLU bit for bit (NaN included), the
residual tails and the gate (LeakyReLU exact, sigmoid against ATen's own measured error), FlowNet's bias_act and its two-channel
backward kernels per element, the fused affine regulariser per cell.  Every destination is pre-filled with NaN (or is a view into a
NaN-filled buffer whose surroundings must stay NaN): an element the sweep never wrote, or a write outside the view, fails.  Shapes
reach every route -- vector / scalar, a misaligned start, one sweep past the grid cap, every flow-head tile width -- as
tests/test_small_kernel_bounds_cpu.py resolves them.  Run with ``-m gpu`` on the MI355X."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import small_kernel_bounds as sk
from test_gpu_conv_bounds import _not_ran, _ran, _scoped

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
BASIC = ("iid", "integers")


def _call(name, *args):
    from ffwm_amd import _lib
    _lib.check(getattr(_lib.load(), name)(*args, _lib.F32, torch.cuda.current_stream().cuda_stream), name)


def _nan_like(t):
    return torch.full_like(t, NAN)


def _placed(t, offset):
    """t on the GPU, `offset` elements into its buffer when offset > 0."""
    return sk.offset_view(t.to(DEV), offset) if offset else t.to(DEV)


def _dest(shape, stride, offset):
    """A destination view [B, C, H, W] with batch stride `stride`, `offset` elements into a NaN-filled buffer; check(): everything
    outside the view still NaN."""
    B, C, H, W = shape
    buf = torch.full((offset + B * stride + 8,), NAN, device=DEV)
    view = buf.as_strided(shape, (stride, H * W, W, 1), offset)
    inside = torch.zeros(buf.shape, dtype=torch.bool, device=DEV)
    inside.as_strided(shape, (stride, H * W, W, 1), offset).fill_(True)

    def check():
        assert bool(torch.isnan(buf[~inside]).all()), "a write outside the destination view"
    return view, check


# ------------------------------------------------------------------------------------------------ 1. mfm and bias + ReLU
def _cases(table, kinds, nonfinite_big, bias_options):
    """Every family (with and without a bias) at the small shapes; iid and one non-finite family, with a bias, past the grid cap."""
    out = []
    for shape, offset, route, past in table:
        for kind in (("iid", nonfinite_big) if past else kinds):
            for with_bias in (bias_options[-1:] if past else bias_options):
                out.append(pytest.param(shape, offset, kind, with_bias, id="%s-off%d-%s-%s-%s%s" % (
                    "x".join(map(str, shape)), offset, route, "past" if past else "one_sweep", kind, "-bias" if with_bias else "")))
    return out


@pytest.mark.parametrize("shape,offset,kind,with_bias", _cases(sk.MFM_SHAPES, sk.MFM_KINDS, "nan_both", (False, True)))
def test_mfm_bit_for_bit(shape, offset, kind, with_bias):
    """y and d(x) equal to torch.max(*split(x + bias)) and its autograd on the CPU: same NaN positions, equal elsewhere."""
    from ffwm_amd.external_function import MaxFeatureMapFunction
    x, bias, go = sk.mfm_inputs(kind, shape, sum(shape), with_bias)
    y_ref, dx_ref, db_ref = sk.mfm_reference(x, bias, go)
    xd, bd, god = _placed(x, offset), (None if bias is None else bias.to(DEV)), go.to(DEV)
    B, C, HW = shape[0], shape[1] // 2, shape[2] * shape[3]
    y, dx = _nan_like(god), torch.full(shape, NAN, device=DEV)
    with _scoped() as rows:
        _call("ffwm_mfm_forward", xd.data_ptr(), None if bd is None else bd.data_ptr(), y.data_ptr(), B, C, HW)
        _call("ffwm_mfm_backward", xd.data_ptr(), None if bd is None else bd.data_ptr(), god.data_ptr(), dx.data_ptr(), B, C, HW)
    _ran(rows, "mfm_fwd", "mfm_bwd")
    what = "mfm %s offset %d %s" % (shape, offset, kind)
    sk.assert_same(y, y_ref, what + " y")
    sk.assert_same(dx, dx_ref, what + " d(x)")
    if x.numel() <= 1 << 16:                                      # through the autograd Function: the same values, and d(bias)
        xa = xd.clone().requires_grad_(True) if not offset else sk.offset_view(x.to(DEV), offset).requires_grad_(True)
        ba = None if bd is None else bd.clone().requires_grad_(True)
        out = MaxFeatureMapFunction.apply(xa, ba)
        out.backward(god)
        sk.assert_same(out, y_ref, what + " Function y")
        sk.assert_same(xa.grad, dx_ref, what + " Function d(x)")
        if ba is not None and bool(torch.isfinite(db_ref).all()):
            d = (ba.grad.cpu() - db_ref).abs().max().item()
            assert d <= 1e-5 * (1 + db_ref.abs().max().item()), (what, d)


@pytest.mark.parametrize("shape,offset,kind,_with_bias", _cases(sk.RELU_SHAPES, sk.RELU_KINDS, "nan", (True,)))
def test_bias_relu_bit_for_bit(shape, offset, kind, _with_bias):
    """relu(h + bias) and, through BiasReLUFunction, d(h) from y: equal to the CPU composition, NaN where it has NaN."""
    from ffwm_amd.external_function import BiasReLUFunction
    h, bias, go = sk.relu_inputs(kind, shape, sum(shape) + 2)
    y_ref, dh_ref, db_ref = sk.relu_reference(h, bias, go)
    hd, bd = _placed(h, offset), bias.to(DEV)
    B, C, HW = shape[0], shape[1], shape[2] * shape[3]
    y = torch.full(shape, NAN, device=DEV)
    with _scoped() as rows:
        _call("ffwm_bias_relu_forward", hd.data_ptr(), bd.data_ptr(), y.data_ptr(), B, C, HW)
    _ran(rows, "bias_relu_fwd")
    what = "bias_relu %s offset %d %s" % (shape, offset, kind)
    sk.assert_same(y, y_ref, what + " y")
    inplace = _placed(h, offset)
    _call("ffwm_bias_relu_forward", inplace.data_ptr(), bd.data_ptr(), inplace.data_ptr(), B, C, HW)
    sk.assert_same(inplace, y_ref, what + " in place")
    ha = (sk.offset_view(h.to(DEV), offset) if offset else h.to(DEV)).requires_grad_(True)
    ba = bd.clone().requires_grad_(True)
    out = BiasReLUFunction.apply(ha, ba)
    out.backward(go.to(DEV))
    sk.assert_same(out, y_ref, what + " Function y")
    sk.assert_same(ha.grad, dh_ref, what + " d(h)")
    if bool(torch.isfinite(db_ref).all()):
        d = (ba.grad.cpu() - db_ref).abs().max().item()
        assert d <= 1e-5 * (1 + db_ref.abs().max().item()), (what, d)


# ------------------------------------------------------------------------------------------------ 2. residual tails and gate
def _residual_inputs(shape, seed):
    n = int(torch.Size(shape).numel())
    a, b = sk.sweep_z(n, seed)
    return n, a, b, sk.mixed_scale(n, seed + 1), sk.mixed_scale(n, seed + 2)


@pytest.mark.parametrize("shape", sk.RESIDUAL_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_leaky_relu_tail_bit_for_bit(shape):
    """add_act LeakyReLU forward and backward equal to ATen's fp32 composition, the kink (+-0, the smallest normals), NaN and the tail
    lane of 1, 2, 3 elements included."""
    n, a, b, _, g = _residual_inputs(shape, 21)
    y_ref, dz_ref = sk.leaky_reference(a, b, g, 0.2)
    ad, bd, gd = a.to(DEV), b.to(DEV), g.to(DEV)
    y, dz = _nan_like(ad), _nan_like(ad)
    with _scoped() as rows:
        _call("ffwm_add_act_forward", ad.data_ptr(), bd.data_ptr(), y.data_ptr(), n, 1, 0.2)
        _call("ffwm_add_act_backward", y.data_ptr(), gd.data_ptr(), dz.data_ptr(), n, 1, 0.2)
    _ran(rows, "add_act_fwd", "add_act_bwd")
    sk.assert_same(y, y_ref, "add_act lrelu %s y" % (shape,))
    sk.assert_same(dz, dz_ref, "add_act lrelu %s dz" % (shape,))


@pytest.mark.parametrize("shape", sk.RESIDUAL_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_sigmoid_paths_against_aten_on_the_device(shape):
    """add_act sigmoid, sigmoid_gate forward / backward.  Inside -87 <= z <= 87 the kernel's worst relative error against float64 may
    exceed that of ATen's fp32 composition on the same device by 2 u; outside, and for +-inf and NaN, it equals ATen bit for bit.  The
    products are held to one rounding each (tests/small_kernel_bounds.py).
    Measured on the MI355X (n = 2 162 688 and 2 116 797, a + b exact): kernel 2.193 u, ATen 2.193 u, allowed 4.193 u, for add_act, the
    gate and the strided gate alike; (2, 3, 4, 6): 1.475 u both.  The products: y 1.00, dx 1.00 (one rounding each: the bound is
    tight), gate dz 0.82, add_act dz 0.87 of their bounds."""
    n, a, b, x, g = _residual_inputs(shape, 23)
    big = n > 1000
    ad, bd, xd, gd = a.to(DEV), b.to(DEV), x.to(DEV), g.to(DEV)
    aten = torch.sigmoid(ad + bd)
    y, dz = _nan_like(ad), _nan_like(ad)
    _call("ffwm_add_act_forward", ad.data_ptr(), bd.data_ptr(), y.data_ptr(), n, 3, 0.0)
    _call("ffwm_add_act_backward", y.data_ptr(), gd.data_ptr(), dz.data_ptr(), n, 3, 0.0)
    what = "add_act sigmoid %s" % (shape,)
    sk.check_sigmoid(y, aten, a, b, what, need_outside=big)
    sk.check_product(dz, sk.sigmoid_backward_ref(y, g), 3, what + " dz")
    att, gy, gz, gx = _nan_like(ad), _nan_like(ad), _nan_like(ad), _nan_like(ad)
    with _scoped() as rows:
        _call("ffwm_sigmoid_gate_forward", ad.data_ptr(), bd.data_ptr(), xd.data_ptr(), att.data_ptr(), gy.data_ptr(), n)
        _call("ffwm_sigmoid_gate_backward", xd.data_ptr(), att.data_ptr(), gd.data_ptr(), gz.data_ptr(), gx.data_ptr(), n)
    _ran(rows, "sigmoid_gate_fwd", "sigmoid_gate_bwd")
    what = "sigmoid_gate %s" % (shape,)
    sk.check_sigmoid(att, aten, a, b, what, need_outside=big)
    sk.assert_same(att, y, what + ": the gate's att and add_act's sigmoid are the same arithmetic")
    sk.check_product(gy, x.double() * att.cpu().double(), 1, what + " y")
    dz_ref, dx_ref = sk.gate_backward_refs(x, att, g)
    sk.check_product(gz, dz_ref, 4, what + " dz")
    sk.check_product(gx, dx_ref, 1, what + " dx")


@pytest.mark.parametrize("want_att", [True, False])
@pytest.mark.parametrize("shape,route", sk.GATE_STRIDED_SHAPES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_sigmoid_gate_strided_past_the_grid_cap(shape, route, want_att):
    """gate_strided_kernel past 524 288 threads into a guarded view: ffwm_sigmoid_gate_forward's values bit for bit, att within the
    sigmoid yardstick."""
    from ffwm_amd import ops
    B, C, H, W = shape
    n, a, b, x, _ = _residual_inputs(shape, 25)
    ad, bd, xd = (t.view(shape).to(DEV) for t in (a, b, x))
    y_ref, att_ref = ops.sigmoid_gate_forward(ad, bd, xd)
    view, check = _dest(shape, (C + 5) * H * W, 2 * H * W)
    with _scoped() as rows:
        y, att = ops.sigmoid_gate_forward_strided(ad, bd, xd, out=view, want_att=want_att)
    _ran(rows, "netg_sigmoid_gate")
    check()
    sk.assert_same(y, y_ref, "gate strided %s y" % route)
    if want_att:
        sk.assert_same(att, att_ref, "gate strided %s att" % route)
        sk.check_sigmoid(att.reshape(-1), torch.sigmoid(ad + bd).reshape(-1), a, b, "gate strided %s" % route)
    else:
        assert att is None


def test_residual_aliasing_contracts():
    """'y may alias a or b', 'grad_z may alias grad_y', 'att may alias a or b' (residual.hip): bit-equal to the call with separate
    tensors.  Through the C ABI: ops always allocates."""
    n = 4 * 70000 + 3                                             # float4 lanes over more than one block, and a tail of 3
    a, b = sk.sweep_z(n, 27)
    x, g = sk.mixed_scale(n, 28), sk.mixed_scale(n, 29)
    ad, bd, xd, gd = a.to(DEV), b.to(DEV), x.to(DEV), g.to(DEV)
    for act, slope in ((1, 0.2), (3, 0.0)):
        y = _nan_like(ad)
        _call("ffwm_add_act_forward", ad.data_ptr(), bd.data_ptr(), y.data_ptr(), n, act, slope)
        for which in (0, 1):
            a2, b2 = ad.clone(), bd.clone()
            dst = (a2, b2)[which]
            _call("ffwm_add_act_forward", a2.data_ptr(), b2.data_ptr(), dst.data_ptr(), n, act, slope)
            sk.assert_same(dst, y, "add_act act %d: y aliases %s" % (act, "ab"[which]))
        dz, g2 = _nan_like(ad), gd.clone()
        _call("ffwm_add_act_backward", y.data_ptr(), gd.data_ptr(), dz.data_ptr(), n, act, slope)
        _call("ffwm_add_act_backward", y.data_ptr(), g2.data_ptr(), g2.data_ptr(), n, act, slope)
        sk.assert_same(g2, dz, "add_act act %d: grad_z aliases grad_y" % act)
    att, y = _nan_like(ad), _nan_like(ad)
    _call("ffwm_sigmoid_gate_forward", ad.data_ptr(), bd.data_ptr(), xd.data_ptr(), att.data_ptr(), y.data_ptr(), n)
    for which in (0, 1):
        a2, b2, y2 = ad.clone(), bd.clone(), _nan_like(ad)
        dst = (a2, b2)[which]
        _call("ffwm_sigmoid_gate_forward", a2.data_ptr(), b2.data_ptr(), xd.data_ptr(), dst.data_ptr(), y2.data_ptr(), n)
        sk.assert_same(dst, att, "sigmoid_gate: att aliases %s" % "ab"[which])
        sk.assert_same(y2, y, "sigmoid_gate: y with att aliasing %s" % "ab"[which])


class _TinyResidual(nn.Module):
    """What residual.gated looks for in netG's att_i: blocks, input and a sigmoid."""

    def __init__(self):
        super().__init__()
        self.blocks, self.input, self.activ = nn.Identity(), nn.Identity(), nn.Sigmoid()

    def forward(self, h):
        return self.activ(self.blocks(h) + self.input(h))


def test_residual_falls_back_for_a_view_at_an_odd_offset():
    """add_act / gated promise the PyTorch composition when the kernel does not apply: a contiguous view one element into its buffer
    is not 16-byte aligned, which the C entry refuses."""
    from ffwm_amd import residual
    shape = (2, 3, 4, 6)
    gen = torch.Generator().manual_seed(31)
    a, b, go = (torch.randn(shape, generator=gen) for _ in range(3))
    ref_in = a.clone().requires_grad_(True)
    ref = F.leaky_relu(ref_in + b, 0.2)
    ref.backward(go)
    act = nn.LeakyReLU(0.2)
    for mis_a, mis_b, mis_g in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)):
        ad = _placed(a, mis_a).requires_grad_(True)
        bd, gd = _placed(b, mis_b), _placed(go, mis_g)
        assert residual._kernel_ok(ad, bd) == (not (mis_a or mis_b))
        with _scoped() as rows:
            y = residual.add_act(ad, bd, act)
            y.backward(gd)
        if mis_a or mis_b:
            _not_ran(rows, "add_act_fwd", "add_act_bwd")
        else:
            _ran(rows, "add_act_fwd", "add_act_bwd")
        assert torch.equal(y.detach().cpu(), ref.detach()) and torch.equal(ad.grad.cpu(), ref_in.grad), (mis_a, mis_b, mis_g)
    att_module = nn.Sequential(nn.Identity(), _TinyResidual())
    for mis in (1, 0):
        skip = _placed(a, mis)
        with _scoped() as rows:
            y, att = residual.gated(att_module, skip)
        assert ("sigmoid_gate_fwd" in rows) == (not mis), rows
        att_ref = torch.sigmoid(skip + skip)
        if mis:                                                   # the composition itself
            assert torch.equal(att, att_ref) and torch.equal(y, skip * att_ref)
        else:                                                     # the kernel (held to its own yardstick above)
            assert torch.allclose(att, att_ref, rtol=1e-5, atol=0) and torch.allclose(y, skip * att_ref, rtol=1e-5, atol=0)


# ------------------------------------------------------------------------------------------------ 3. FlowNet's small layers
def _bias_act_params():
    out = []
    for name, case in sk.BIAS_ACT_CASES.items():
        for act in (0, 1, 2):
            out.append(pytest.param(name, act, id="%s-act%d" % (name, act)))
    return out


@pytest.mark.parametrize("name,act", _bias_act_params())
def test_bias_act_destinations_and_routes(name, act):
    """act none / LeakyReLU bit-equal to the composition, tanh within 4 ulps of float64 tanh(fl(h + b)); in place, into a guarded
    slice, into two destinations with different batch strides, into the second only; the scalar route three ways; past the cap."""
    from ffwm_amd import flownet_eval
    shape, ydesc, y2desc, with_bias, route, past = sk.BIAS_ACT_CASES[name]
    assert sk.bias_act_case_route(name)[::2] == (route, past)
    B, C, H, W = shape
    h = sk.activations("iid", shape, 33 + C) * 3
    bias = torch.randn(C, generator=torch.Generator().manual_seed(34)) if with_bias else None
    ref = sk.bias_act_reference(h, bias, act, 0.2)
    hd, bd = h.to(DEV), (None if bias is None else bias.to(DEV))
    checks = []
    if ydesc == "inplace":
        y = None
    elif ydesc is None:
        y = None
    else:
        y, c = _dest(shape, *ydesc)
        checks.append(c)
    y2 = None
    if y2desc is not None:
        y2, c = _dest(shape, *y2desc)
        checks.append(c)
    with _scoped() as rows:
        out = flownet_eval.bias_act(hd, bd, act, y=y, y2=y2, slope=0.2)
    _ran(rows, "flownet_bias_act")
    for c in checks:
        c()
    for got in ([hd] if ydesc == "inplace" else []) + [t for t in (y, y2) if t is not None] + [out]:
        if act == 2:
            ref.check(got, "bias_act tanh %s" % name)
        else:
            sk.assert_same(got, ref, "bias_act %s act %d" % (name, act))


def _head_bwd_params():
    out = []
    for shape in sk.FLOW_HEAD_BWD_SHAPES:
        for kind in (sk.cb.FAMILIES if shape == (4, 70, 19, 23) else BASIC):
            for ykind in (sk.HEAD_Y_KINDS if kind == "iid" else ("moderate",)):
                out.append(pytest.param(shape, kind, ykind, id="%s-P%d-%s-%s" % ("x".join(map(str, shape)), sk.flow_head_tile(shape[0], shape[2] * shape[3]), kind, ykind)))
    return out


@pytest.mark.parametrize("shape,kind,ykind", _head_bwd_params())
def test_flow_head_backward_per_element(shape, kind, ykind):
    """ffwm_flow_head_backward from a given fp32 y: grad_z within 3 u |go| and grad_x within (18 + 4) u mag of float64 (x SAFETY), at
    every tile width; y = +-1 gives grad_z = 0 exactly; integers with y = 0 are exact."""
    B, C, H, W = shape
    go = sk.grad_outputs(kind, (B, 2, H, W), 40 + C)
    w, _ = sk.weights(kind, (2, C, 3, 3), 41 + C)
    y = sk.head_outputs("zero" if kind == "integers" else ykind, (B, 2, H, W), 42 + C)
    zb, xb = sk.flow_head_backward_bounds(y, go, w, exact=kind == "integers", what="flow_head_bwd %s %s %s" % (shape, kind, ykind))
    yd, god, wd = y.to(DEV), go.to(DEV), w.to(DEV)
    gz, gx = torch.full((B, 2, H, W), NAN, device=DEV), torch.full(shape, NAN, device=DEV)
    with _scoped() as rows:
        _call("ffwm_flow_head_backward", yd.data_ptr(), god.data_ptr(), wd.data_ptr(), gz.data_ptr(), gx.data_ptr(), B, C, H, W)
    _ran(rows, "flownet_flow_head_bwd")
    zb.check(gz)
    xb.check(gx)
    if ykind == "ones" and kind != "integers":
        assert bool((gz == 0).all())


@pytest.mark.parametrize("kind", sk.cb.FAMILIES)
@pytest.mark.parametrize("shape", [(8, 2, 2), (3, 7, 9), (8, 16, 16), (1, 1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_flow_up_backward_per_element(shape, kind):
    """ffwm_flow_up_backward against float64 conv2d(go, w, stride 2, pad 1), rho_any_order(2 x 16); go is read in place as the last two
    channels of a wider gradient whose other channels hold NaN."""
    B, H, W = shape
    go = sk.grad_outputs(kind, (B, 2, 2 * H, 2 * W), 50 + H)
    w, _ = sk.weights(kind, (2, 2, 4, 4), 51 + H, out_dim=1)
    bound = sk.flow_up_backward_bound(go, w, exact=kind == "integers", what="flow_up_bwd %s %s" % (shape, kind))
    wide = torch.full((B, 7, 2 * H, 2 * W), NAN, device=DEV)
    wide[:, 5:] = go.to(DEV)
    wd = w.to(DEV)
    gx = torch.full((B, 2, H, W), NAN, device=DEV)
    with _scoped() as rows:
        _call("ffwm_flow_up_backward", wide[:, 5:].data_ptr(), wd.data_ptr(), gx.data_ptr(), B, H, W, wide.stride(0))
    _ran(rows, "flownet_flow_up_bwd")
    bound.check(gx)


# ------------------------------------------------------------------------------------------------ 4. fused affine regulariser
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", sk.AFFINE_FLOWS)
@pytest.mark.parametrize("shape", sk.AFFINE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_affine_regularization_per_cell(shape, kind, dtype):
    """The gradient within SAFETY (2 kz^2 + 4) u mag per cell and the loss within its launch-geometry bound, in fp32 and float64; a NaN
    cell reaches exactly the cells within kz - 1 of it and the loss; want_grad=False gives a loss within the same bound."""
    from ffwm_amd import ops
    B, h, w, kz = shape
    flow = sk.affine_flow(kind, B, h, w, 60 + h).to(dtype)
    M = sk.affine_matrix(kz)
    lb, gb = sk.affine_bounds(flow, M, kz, dtype, what="affine %s %s %s" % (shape, kind, str(dtype)[6:]))
    fd = flow.to(DEV)
    with _scoped() as rows:
        loss, grad = ops.affine_regularization(fd, M, kz, want_grad=True)
        loss_only, none = ops.affine_regularization(fd, M, kz, want_grad=False)
    assert rows.get("affine_regularization", 0) == 2 and none is None
    gb.check(grad)
    lb.check(loss)
    lb.check(loss_only, lb.what + " (want_grad=False)")
    if kind == "nan_cell":
        yy, xx = h // 2, w - 2
        expect = torch.zeros(flow.shape, dtype=torch.bool)
        expect[B - 1, 1, max(yy - kz + 1, 0):yy + kz, max(xx - kz + 1, 0):xx + kz] = True
        assert torch.equal(torch.isnan(grad).cpu(), expect) and bool(torch.isnan(loss)) and bool(torch.isnan(loss_only))
    else:
        assert bool(torch.isfinite(grad).all())

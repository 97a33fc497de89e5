"""The training half of --crop without a GPU: the adjoint's reference and bound (tests/identity_train_bounds.py), losses.IdentityLoss
against the reference's own, the C ABI's refusals and the defaults of the new options."""
import ctypes
import inspect
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import identity_bounds as ib  # noqa: E402
import identity_train_bounds as tb  # noqa: E402


def test_matrices_reproduce_the_crop_reference():
    """out = A_y gray A_x^T is identity_bounds.crop_reference to float64 rounding, for the crop and for its two wrong variants; the
    counts and the frame the bound's docstring states are those of the matrices."""
    img = torch.randn(2, 3, 128, 128, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    gray = img.mean(1, keepdim=True)
    for kw in ({}, {"row_origin": ib.COL_ORIGIN}, {"align_corners": True}):
        ay, ax = tb.crop_matrices(**kw)
        got = torch.einsum("oy,bcyx,px->bcop", ay, gray, ax)
        assert (got - ib.crop_reference(img, **kw)).abs().max().item() <= 1e-13 * 16
    assert ib.crop_taps_inside()
    assert (tb.A_Y >= 0).all() and (tb.A_X >= 0).all()
    assert (tb.A_Y.sum(1) - 1).abs().max().item() <= 1e-15 and (tb.A_X.sum(1) - 1).abs().max().item() <= 1e-15
    assert (tb.N_Y, tb.N_X, tb.N_TOUCH) == (4, 4, 16)
    assert tb.ROWS_INSIDE.nonzero().flatten().tolist() == list(range(27, 127))
    assert tb.COLS_INSIDE.nonzero().flatten().tolist() == list(range(14, 114))
    # no source coordinate sits near an integer: a coordinate rounding never moves a tap to another cell
    for c in ib.crop_coordinates():
        assert (c - c.round()).abs().min().item() >= 1.0 / 194 - 1e-12
    # the adjoint is the adjoint: <A x, g> == <x, A^T g> in float64
    g = tb.random_g(2).double()
    lhs = (torch.einsum("oy,bcyx,px->bcop", tb.A_Y, gray, tb.A_X) * g).sum()
    rhs = (img * tb.crop_adjoint_reference(g, 3)).sum()
    assert abs(float(lhs - rhs)) <= 1e-12 * float((gray.abs() * tb.crop_adjoint_reference(g.abs(), 1)).sum())


def _aten_adjoint(g, cin):
    from ffwm_amd.identity_eval import torch_identity_input
    x = torch.zeros(g.shape[0], cin, 128, 128, requires_grad=True)
    torch_identity_input(x, crop=True).backward(g)
    return x.grad


@pytest.mark.parametrize("name", ["random"] + sorted(tb.ONE_HOT))
def test_adjoint_bound_holds_for_aten(name):
    """ATen's own fp32 autograd of the composition (grid_sample and upsample_bilinear2d backward, another summation order than the
    kernel's) lies inside the bound, and is exactly 0 where no output touches."""
    cin = 3 if name == "random" else 1
    g = tb.random_g(2) if name == "random" else tb.one_hot(name)
    ref, bound = tb.crop_adjoint_bound(g, cin)
    got = _aten_adjoint(g, cin)
    r = tb.worst_ratio(got, ref, bound)
    print("adjoint bound, ATen fp32 autograd, %s: error / bound %.3g" % (name, r))
    assert r <= 1.0
    assert (bound[:, :, ~tb.ROWS_INSIDE] == 0).all() and (bound[:, :, :, ~tb.COLS_INSIDE] == 0).all()
    assert (bound[:, :, 27:127, 14:114] > 0).any()
    if name != "random":
        oy, ox = tb.ONE_HOT[name]
        assert abs(float(ref.sum()) - 1.0) <= 1e-14 and int((ref != 0).sum()) == int((tb.A_Y[oy] != 0).sum() * (tb.A_X[ox] != 0).sum())


def test_adjoint_bound_breaks_for_the_wrong_variants():
    g = tb.random_g(2)
    ref, bound = tb.crop_adjoint_bound(g, 3)
    floor = bound[bound > 0].min()
    factors = {}
    for what, kw in (("row centre 64", {"row_origin": ib.COL_ORIGIN}), ("align_corners=True", {"align_corners": True})):
        wrong = tb.crop_adjoint_reference(g, 3, tb.crop_matrices(**kw))
        factors[what] = float(((wrong - ref).abs() / bound.clamp(min=floor)).max())
    print("adjoint bound, wrong variants (error / bound): " + ", ".join("%s %.3g" % kv for kv in factors.items()))
    assert all(f >= 100.0 for f in factors.values())


@pytest.mark.parametrize("crop", [False, True])
def test_identity_loss_equals_the_reference(crop):
    """losses.IdentityLoss in float64 on the CPU against the reference's own run (the fixture): the same loss and the same d loss / d out
    to 1e-9 of the fixture's largest element."""
    from ffwm_amd import losses
    fx = tb.loss_fixture()
    out, gt = tb.loss_inputs()
    key = "crop" if crop else "plain"
    assert float(fx["grad_spread_" + key]) <= 1e-18
    x = out.clone().requires_grad_(True)
    mod = losses.IdentityLoss(tb.StandIn(), crop=crop)
    loss = mod(x, gt)
    loss.backward()
    loss = loss.detach()
    err_l = abs(float(loss) - float(fx["loss_" + key]))
    err_g = float((x.grad - fx["grad_" + key]).abs().max())
    print("IdentityLoss crop=%s: loss %.15g, |loss - fixture| %.3g, max |grad - fixture| %.3g of %.3g" % (
        crop, float(loss), err_l, err_g, float(fx["grad_" + key].abs().max())))
    assert err_l <= 1e-9 * abs(float(fx["loss_" + key]))
    assert err_g <= 1e-9 * float(fx["grad_" + key].abs().max())
    assert not gt.requires_grad
    # the restatement the GPU tests compare with agrees with the fixture within the float32 grid's coordinate error, and the inputs
    # keep every feature difference clear of zero
    assert abs(float(tb.reference_loss(out, gt, crop)) - float(fx["loss_" + key])) <= tb.loss_tolerance(out, gt, crop)
    assert tb.signs_are_safe(out, gt, crop)
    assert tb.loss_tolerance(out, gt, crop) <= 0.01 * float(fx["loss_" + key])


def test_identity_loss_mirrors_the_reference_interface():
    from ffwm_amd import losses
    from ffwm_amd.identity_eval import crop_grid
    sig = inspect.signature(losses.IdentityLoss.__init__)
    assert list(sig.parameters) == ["self", "lightcnn", "crop"] and sig.parameters["crop"].default is False
    mod = losses.IdentityLoss(tb.StandIn())
    assert mod.crop is False and isinstance(mod.criterionL1, torch.nn.L1Loss)
    assert torch.equal(mod.build_grid(2, 98), crop_grid(2))
    assert mod.build_grid(1, 98).shape == (1, 2, 98, 98)
    assert "commute" in losses.IdentityLoss.__doc__
    # float32 on the CPU is the PyTorch composition, differentiable
    out, gt = (t.float() for t in tb.loss_inputs())
    x = out.clone().requires_grad_(True)
    loss = losses.IdentityLoss(tb.StandIn(torch.float32), crop=True)(x, gt)
    loss.backward()
    assert abs(float(loss.detach()) - float(tb.loss_fixture()["loss_crop"])) <= 2 * tb.loss_tolerance(out, gt, True)
    with pytest.raises(ValueError):
        losses.IdentityLoss(tb.StandIn(torch.float32), crop=True)(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 64))


def test_new_symbol_is_declared_and_bound():
    from ffwm_amd import _lib, build
    text = open(os.path.join(os.path.dirname(HERE), "include", "ffwm_hip.h")).read()
    assert re.search(r"\bffwm_identity_input_backward\s*\(", text)
    assert "ffwm_identity_input_backward" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 5
    build.build()
    assert hasattr(_lib.load(), "ffwm_identity_input_backward")


def test_argument_errors_come_before_any_launch():
    """No device here: every refusal below is decided on the host."""
    from ffwm_amd import build, _lib
    build.build()
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = lib.ffwm_identity_input_backward
    assert f(None, p, 1, 3, 4, 4, 0, 0, None) == -1 and b"NULL" in lib.ffwm_last_error()
    assert f(p, None, 1, 3, 4, 4, 0, 0, None) == -1 and b"NULL" in lib.ffwm_last_error()
    assert f(p, p, 1, 3, 4, 4, 0, 1, None) == -2
    assert f(p, p, 1, 3, 64, 64, 1, 0, None) == -1 and b"128" in lib.ffwm_last_error()
    assert f(p, p, 1, 3, 4, 4, 2, 0, None) == -1 and b"crop" in lib.ffwm_last_error()
    assert f(p, p, 1, 0, 4, 4, 0, 0, None) == -1
    assert f(p, p, 65536, 3, 128, 128, 1, 0, None) == -3 and b"too large" in lib.ffwm_last_error()
    assert f(p, p, 1, 3, 1 << 20, 4, 0, 0, None) == -3


def test_ops_refuse_what_the_kernel_does_not_serve():
    from ffwm_amd import ops
    g = torch.zeros(1, 1, 128, 128)
    with pytest.raises(NotImplementedError):
        ops.identity_input_backward(g, 3)                       # a CPU tensor
    sig = inspect.signature(ops.identity_input_backward)
    assert list(sig.parameters) == ["grad_out", "cin", "crop", "out"] and sig.parameters["crop"].default is False
    assert list(inspect.signature(ops.identity_input).parameters) == ["img", "crop", "out"]


def test_crop_defaults_to_false():
    from ffwm_amd import losses, trainer
    assert inspect.signature(trainer.FFWMTrainer.__init__).parameters["crop"].default is False
    assert inspect.signature(losses.IdentityLoss.__init__).parameters["crop"].default is False
    assert "opt.crop" in trainer.FFWMTrainer.identity_feature.__doc__


def _bare_trainer(net, crop):
    """An FFWMTrainer with nothing but what the identity losses read."""
    from ffwm_amd import trainer
    t = trainer.FFWMTrainer.__new__(trainer.FFWMTrainer)
    t.lightCNN, t.crop = net, crop
    return t


def test_identity_many_without_crop_is_what_it_was():
    """crop=False on the CPU: identity_many, restated here as it stood before the option, bit for bit -- values and gradients."""
    net = tb.StandIn(torch.float32)
    gen = torch.Generator().manual_seed(4)
    a, b, gt = (torch.rand(2, 3, 128, 128, generator=gen) for _ in range(3))

    def before(outs, weights):
        with torch.no_grad():
            _, fc_g, pool_g = net(gt.mean(1, keepdim=True))
        _, fc_o, pool_o = net(torch.cat([u.mean(1, keepdim=True) for u in outs], 0))
        total = 0
        for i, w in enumerate(weights):
            sl = slice(i * 2, (i + 1) * 2)
            total = total + w * (F.l1_loss(fc_o[sl], fc_g) + F.l1_loss(pool_o[sl], pool_g))
        return total
    t = _bare_trainer(net, False)
    a1, b1, a2, b2 = (u.clone().requires_grad_(True) for u in (a, b, a, b))
    got, want = t.identity_many((a1, b1), gt, (0.5, 1.0)), before((a2, b2), (0.5, 1.0))
    assert torch.equal(got, want)
    got.backward()
    want.backward()
    assert torch.equal(a1.grad, a2.grad) and torch.equal(b1.grad, b2.grad)
    # the same tensor twice runs once, with the weights added
    a3, a4 = a.clone().requires_grad_(True), a.clone().requires_grad_(True)
    assert torch.equal(t.identity_many((a3, a3), gt, (0.5, 1.0)), before((a4,), (1.5,)))
    assert torch.equal(t.identity(a, gt), F.l1_loss(net(a.mean(1, keepdim=True))[1], net(gt.mean(1, keepdim=True))[1])
                       + F.l1_loss(net(a.mean(1, keepdim=True))[2], net(gt.mean(1, keepdim=True))[2]))


def test_identity_many_with_crop_on_the_cpu():
    """crop=True on the CPU (the PyTorch composition): every LightCNN input is the crop -- the float64 restatement within the tolerance."""
    net = tb.StandIn(torch.float32)
    out, gt = (u.float() for u in tb.loss_inputs())
    t = _bare_trainer(net, True)
    want = 1.5 * float(tb.reference_loss(out, gt, True))
    got = float(t.identity_many((out, out), gt, (0.5, 1.0)))
    assert abs(got - want) <= 1.5 * tb.loss_tolerance(out, gt, True)
    assert abs(float(t.identity(out, gt)) - want / 1.5) <= tb.loss_tolerance(out, gt, True)
    assert abs(got - 1.5 * float(tb.reference_loss(out, gt, False))) >= 10 * tb.loss_tolerance(out, gt, True)      # not the plain mean

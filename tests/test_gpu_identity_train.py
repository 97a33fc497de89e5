"""ffwm_identity_input_backward (csrc/lightcnn_eval.hip), IdentityInputFunction, losses.IdentityLoss and FFWMTrainer(crop=True) on the
MI355X -- run with ``-m gpu``.  References, bounds and input families: tests/identity_train_bounds.py."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import identity_bounds as ib  # noqa: E402
import identity_train_bounds as tb  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
G_NAMES = ["random"] + sorted(tb.ONE_HOT)


def _g(name, B):
    return tb.random_g(B, seed=7 + B) if name == "random" else tb.one_hot(name, B)


def _launches(fn):
    """-> {kernel name: launches} of the library's kernels that fn() issues."""
    from ffwm_amd import _lib
    torch.cuda.synchronize()
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        rows = _lib.prof_collect()
    finally:
        _lib.prof_enable(False)
        _lib.prof_reset()
    return {k: v["launches"] for k, v in rows.items()}


# ---------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("name", G_NAMES)
@pytest.mark.parametrize("B,cin", [(1, 1), (2, 3), (3, 3)])
def test_crop_backward_against_the_float64_adjoint(B, cin, name):
    """Per element within the derived bound, into a batch slice of a NaN-guarded wider buffer; exact zeros outside the crop."""
    from ffwm_amd import ops
    g = _g(name, B)
    ref, bound = tb.crop_adjoint_bound(g, cin)
    buf = torch.full((1 + B + 1, cin, 128, 128), NAN, device=DEV)
    got = ops.identity_input_backward(g.to(DEV), cin, crop=True, out=buf[1:1 + B])
    assert got.data_ptr() == buf[1:1 + B].data_ptr() and got.shape == (B, cin, 128, 128)
    assert torch.isnan(buf[:1]).all() and torch.isnan(buf[1 + B:]).all(), "a write outside the destination"
    r = tb.worst_ratio(got, ref, bound)
    print("identity_input_backward crop B %d Cin %d g %s: error / bound %.3g" % (B, cin, name, r))
    assert r <= 1.0
    got = got.cpu()
    assert (got[:, :, ~tb.ROWS_INSIDE] == 0).all() and (got[:, :, :, ~tb.COLS_INSIDE] == 0).all()
    assert not torch.isnan(got).any()
    for c in range(1, cin):
        assert torch.equal(got[:, c], got[:, 0])
    fresh = ops.identity_input_backward(g.to(DEV), cin, crop=True)
    assert torch.equal(fresh.cpu(), got), "two calls differ"


def test_crop_backward_exactness():
    from ffwm_amd import ops
    zero = ops.identity_input_backward(torch.zeros(2, 1, 128, 128, device=DEV), 3, crop=True)
    assert (zero == 0).all()
    g = tb.random_g(3, seed=12)
    gd = g.to(DEV)
    a, b = ops.identity_input_backward(gd, 3, crop=True), ops.identity_input_backward(gd, 3, crop=True)
    assert torch.equal(a, b)                                    # bit for bit from run to run
    a = a.cpu()
    frame = torch.ones(128, 128, dtype=torch.bool)
    frame[27:127, 14:114] = False                               # rows 0 .. 26 and 127, columns 0 .. 13 and 114 .. 127
    assert (a[:, :, frame] == 0).all() and (a[:, :, ~frame] != 0).any()
    # the weights of every output sum to 1: nothing of g is lost or made
    diff, tol = abs(float(a.double().sum() - g.double().sum())), tb.sum_rule_tolerance(g, 3)
    print("sum rule: |sum(grad_img) - sum(g)| %.3g, tolerance %.3g" % (diff, tol))
    assert diff <= tol
    one = tb.one_hot("centre")
    s = float(ops.identity_input_backward(one.to(DEV), 1, crop=True).double().sum().cpu())
    assert abs(s - 1.0) <= tb.sum_rule_tolerance(one, 1)


def test_forward_and_backward_are_adjoint_on_the_device():
    """<identity_input(x, crop), g> and <x, backward(g)>, both summed in float64 on the host, differ by no more than the forward's
    bound weighed with |g| plus the backward's weighed with |x|."""
    from ffwm_amd import ops
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(2, 3, 128, 128, generator=gen)
    g = torch.randn(2, 1, 128, 128, generator=gen)
    y = ops.identity_input(x.to(DEV), crop=True).cpu().double()
    gx = ops.identity_input_backward(g.to(DEV), 3, crop=True).cpu().double()
    lhs, rhs = float((y * g.double()).sum()), float((x.double() * gx).sum())
    _, fb = ib.crop_bound(x)
    _, bb = tb.crop_adjoint_bound(g, 3)
    tol = float((fb * g.double().abs()).sum() + (bb * x.double().abs()).sum())
    print("adjointness: <Ax, g> %.9g, <x, A^T g> %.9g, difference %.3g, tolerance %.3g" % (lhs, rhs, abs(lhs - rhs), tol))
    assert abs(lhs - rhs) <= tol
    assert abs(lhs) > 1.0                                       # the two sides are not both nothing


@pytest.mark.parametrize("shape", [(1, 3, 5, 7), (2, 3, 128, 128), (2, 1, 6, 10)])
def test_gray_backward_is_the_division(shape):
    """crop = 0: grad_out / Cin in every channel, equal to ATen's division (on the CPU: one correctly rounded division per element) --
    the scalar route (H W % 4 != 0) and the vector route."""
    from ffwm_amd import ops
    B, cin, H, W = shape
    g = torch.randn(B, 1, H, W, generator=torch.Generator().manual_seed(2))
    g.view(-1)[::5] *= 1e-30                                    # tiny values too
    ref = (g / cin).expand(B, cin, H, W).contiguous()
    buf = torch.full((B + 2, cin, H, W), NAN, device=DEV)
    got = ops.identity_input_backward(g.to(DEV), cin, out=buf[1:1 + B])
    assert torch.isnan(buf[:1]).all() and torch.isnan(buf[1 + B:]).all()
    ib.assert_same(got, ref, "identity_input_backward gray %s" % (shape,))
    ib.assert_same(ops.identity_input_backward(g.to(DEV), cin), ref, "fresh destination")


def test_ops_refusals():
    from ffwm_amd import ops
    g = torch.zeros(1, 1, 128, 128, device=DEV)
    with pytest.raises(NotImplementedError):
        ops.identity_input_backward(g.half(), 3)
    with pytest.raises(NotImplementedError):
        ops.identity_input_backward(g.cpu(), 3)
    with pytest.raises(ValueError):
        ops.identity_input_backward(g[:, :, :64, :64].contiguous(), 3, crop=True)
    with pytest.raises(ValueError):
        ops.identity_input_backward(g, 3, out=torch.zeros(1, 2, 128, 128, device=DEV))
    with pytest.raises(ValueError):
        ops.identity_input_backward(torch.zeros(1, 2, 128, 128, device=DEV), 3)
    # identity_input keeps its own
    with pytest.raises(NotImplementedError):
        ops.identity_input(torch.zeros(1, 3, 128, 128, device=DEV).half())
    with pytest.raises(NotImplementedError):
        ops.identity_input(torch.zeros(1, 3, 128, 128))
    with pytest.raises(ValueError):
        ops.identity_input(torch.zeros(1, 3, 64, 64, device=DEV), crop=True)


# ---------------------------------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("crop", [False, True])
def test_function_gradient_is_the_direct_call(crop):
    from ffwm_amd import ops
    from ffwm_amd.external_function import IdentityInputFunction, identity_input_many
    gen = torch.Generator().manual_seed(6)
    img = torch.randn(2, 3, 128, 128, generator=gen).to(DEV).requires_grad_(True)
    w = torch.randn(2, 1, 128, 128, generator=gen).to(DEV)
    y = IdentityInputFunction.apply(img, crop)
    assert y.shape == (2, 1, 128, 128) and torch.equal(y, ops.identity_input(img.detach(), crop))
    counts = _launches(lambda: (w * y).sum().backward())
    assert torch.equal(img.grad, ops.identity_input_backward(w, 3, crop))
    assert counts.get("identity_crop_bwd" if crop else "identity_gray_bwd") == 1
    # nothing is saved but the shape
    assert IdentityInputFunction.apply(img, crop).grad_fn.saved_tensors == ()
    # an input that wants no gradient: no launch
    other = torch.randn(2, 3, 128, 128, generator=gen).to(DEV)
    img.grad = None
    both = identity_input_many([other, img], crop)
    assert both.shape == (4, 1, 128, 128) and torch.equal(both[:2], ops.identity_input(other, crop)) and torch.equal(both[2:], y)
    w4 = torch.cat((w, 2 * w), 0)
    counts = _launches(lambda: (w4 * both).sum().backward())
    assert counts.get("identity_crop_bwd" if crop else "identity_gray_bwd") == 1
    assert torch.equal(img.grad, ops.identity_input_backward(2 * w, 3, crop))

    class Ctx(object):
        needs_input_grad = (False, False)
        cin, crop = 3, True
    counts = _launches(lambda: IdentityInputFunction.backward(Ctx, w))
    assert IdentityInputFunction.backward(Ctx, w) == (None, None) and not counts


# ---------------------------------------------------------------------------------------------------- the loss
def _restated(out, gt, crop, weight=1.0):
    """-> (float64 loss, d loss / d out) of the exact restatement."""
    x = out.double().clone().requires_grad_(True)
    loss = weight * tb.reference_loss(x, gt, crop)
    loss.backward()
    return float(loss.detach()), x.grad


@pytest.mark.parametrize("crop", [False, True])
def test_identity_loss_on_the_device_against_the_fixture(crop):
    """fp32 on the GPU against the reference's float64 run.  Tolerance (tests/identity_train_bounds.py): the input stage's derived
    per-element bound pushed through the stand-in's linear map and the L1 means; the fixture carries the reference's float32 grid, which
    that bound covers too, so the two lie within twice the tolerance of each other.  The gradient: the adjoint's bound at the fixed
    g the loss hands back (the signs of the feature differences are those of the exact evaluation: asserted on the CPU), twice for
    the same reason."""
    from ffwm_amd import losses
    fx = tb.loss_fixture()
    out, gt = tb.loss_inputs()
    key = "crop" if crop else "plain"
    x = out.float().to(DEV).requires_grad_(True)
    mod = losses.IdentityLoss(tb.StandIn(torch.float32, DEV), crop=crop)
    counts = _launches(lambda: mod(x, gt.float().to(DEV)).backward())
    assert counts.get("identity_crop" if crop else "identity_gray") == 2 and counts.get("identity_crop_bwd" if crop else "identity_gray_bwd") == 1
    x.grad = None
    loss = mod(x, gt.float().to(DEV))
    loss.backward()
    tol, gtol = tb.loss_tolerance(out, gt, crop), tb.grad_tolerance(out, crop)
    err = abs(float(loss.detach()) - float(fx["loss_" + key]))
    gerr = (x.grad.cpu().double() - fx["grad_" + key]).abs()
    print("IdentityLoss on the device crop=%s: |loss - fixture| %.3g (tolerance 2 x %.3g), worst gradient error / tolerance %.3g" % (
        crop, err, tol, float((gerr / (2 * gtol).clamp(min=1e-300)).max())))
    assert err <= 2 * tol
    assert (gerr <= 2 * gtol).all()
    assert tol <= 0.01 * float(fx["loss_" + key])


# ---------------------------------------------------------------------------------------------------- the trainer
@pytest.fixture(scope="module")
def trainers():
    from ffwm_amd import trainer
    torch.backends.cudnn.benchmark = False
    return {crop: trainer.FFWMTrainer(DEV, seed=0, ngf=16, crop=crop) for crop in (False, True)}


def test_trainer_identity_many_with_crop(trainers):
    """identity_many with the stand-in for LightCNN: value and gradients against the float64 restatement, and one crop per unique tensor."""
    t = trainers[True]
    assert t.crop is True and trainers[False].crop is False
    out, gt = tb.loss_inputs()
    other = out.flip(3).contiguous()
    assert tb.signs_are_safe(other, gt, True)
    real = t.lightCNN
    t.lightCNN = tb.StandIn(torch.float32, DEV)
    try:
        a, b, gtd = out.float().to(DEV).requires_grad_(True), other.float().to(DEV).requires_grad_(True), gt.float().to(DEV)
        got = t.identity_many((a, b), gtd, (0.5, 1.0))
        got.backward()
        la, ga = _restated(out, gt, True, 0.5)
        lb, gb = _restated(other, gt, True, 1.0)
        tol = 0.5 * tb.loss_tolerance(out, gt, True) + tb.loss_tolerance(other, gt, True)
        print("identity_many crop: %.9g against %.9g, tolerance %.3g" % (float(got.detach()), la + lb, tol))
        assert abs(float(got.detach()) - (la + lb)) <= tol
        gtol = tb.grad_tolerance(out, True)
        assert ((a.grad.cpu().double() - ga).abs() <= 0.5 * gtol).all()
        assert ((b.grad.cpu().double() - gb).abs() <= gtol).all()
        assert (a.grad != 0).any() and (b.grad != 0).any()
        # identity() and identity_feature() take the crop as well
        assert abs(float(t.identity(a.detach(), gtd)) - 2 * la) <= tb.loss_tolerance(out, gt, True)
        # a is b: one crop for the pair, one for the ground truth
        a2 = out.float().to(DEV).requires_grad_(True)
        box = {}
        counts = _launches(lambda: box.update(v=t.identity_many((a2, a2), gtd, (0.5, 1.0))))
        assert counts.get("identity_crop") == 2
        assert abs(float(box["v"].detach()) - 3 * la) <= 1.5 * tb.loss_tolerance(out, gt, True)
        counts = _launches(lambda: t.identity_many((a2, b.detach()), gtd, (0.5, 1.0)))
        assert counts.get("identity_crop") == 3
    finally:
        t.lightCNN = real


def test_trainer_step_with_crop_is_finite_and_not_a_no_op(trainers):
    """One eager step at batch 2 with the real LightCNN: finite losses, and an identity term that differs from the crop=False
    trainer's of the same seed -- the crop reaches the step."""
    import math
    from ffwm_amd import trainer
    batch = trainer.synthetic_batch(2, DEV, seed=3)
    iden = {}
    for (n, p), (_, q) in zip(trainers[True].netG.named_parameters(), trainers[False].netG.named_parameters()):
        assert torch.equal(p, q), n                             # one seed: the two start from the same weights
    for crop in (False, True):
        t = trainers[crop]
        losses = t.step(batch, batch_increment=0)
        torch.cuda.synchronize()
        vals = {k: float(v) for k, v in losses.items()}
        assert all(math.isfinite(v) for v in vals.values()), vals
        iden[crop] = vals["iden"]
    print("train step, iden: crop=False %.6g, crop=True %.6g" % (iden[False], iden[True]))
    assert abs(iden[True] - iden[False]) > 1e-3 * abs(iden[False])
    feat = trainers[True].identity_feature(batch["img_F"])
    plain = trainers[False].identity_feature(batch["img_F"])
    assert feat.shape == plain.shape and not torch.equal(feat, plain)


# ---------------------------------------------------------------------------------------------------- capture
def test_crop_loss_captures_and_replays_bit_for_bit():
    """The crop input stage and the stand-in loss, forward and backward, in one captured graph on the default stream setup: two
    replays equal the eager result bit for bit.  The eager run has a leaf of its own and its graph is gone before the capture: an
    autograd node runs on the stream it was made on, and a gradient accumulator that an eager graph keeps alive would draw that
    stream -- the default one -- into the capture."""
    from ffwm_amd import losses
    out, gt = tb.loss_inputs()
    mod = losses.IdentityLoss(tb.StandIn(torch.float32, DEV), crop=True)
    gtd = gt.float().to(DEV)
    xe = out.float().to(DEV).requires_grad_(True)
    eager = mod(xe, gtd)
    eager.backward()
    want_loss, want_grad = eager.detach().clone(), xe.grad.clone()
    del eager, xe
    x = out.float().to(DEV).requires_grad_(True)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            x.grad = None
            mod(x, gtd).backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    x.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = mod(x, gtd)
        loss.backward()
    loss = loss.detach()
    for _ in range(2):
        x.grad.fill_(NAN)
        loss.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss, want_loss) and torch.equal(x.grad, want_grad)

"""LightCNN fine-tuning on the GPU (trainer.LightCNNTrainer) with the setup of tests/golden/reference_finetune.pt (num_classes 300,
batch 4, the fixture's fill and dropout mask): the step-0 loss, ranks and d(loss)/d(logits) against the bounds of tests/xent_bounds.py
computed from the trainer's own logits; the parameters after the step against the bounds of tests/sgd_bounds.py computed from the
reducer's actual flat gradient; three losses against the reference's; both switches on and off; eager against captured-and-replayed
steps; the learning-rate schedule under replay; one full-size step pair with real dropout."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import finetune_case as fc  # noqa: E402
import sgd_bounds as sb  # noqa: E402
import xent_bounds as xb  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def fx():
    return fc.fixture()


def _xent_bound(tr, batch):
    from ffwm_amd import ops
    case = xb.Case(logits=tr.logits.detach().cpu().contiguous(), target=batch["target"].cpu(), family="trainer")
    return xb.Bound(case, ops.softmax_xent_chunk())


def _sgd_case(opt, p_before, buf_before):
    """One step of FlatSGD as a case of sgd_bounds: the tables the kernel read, the reducer's actual flat gradient."""
    pairs = list(zip(opt.group_lr.cpu().tolist(), opt.group_wd.cpu().tolist()))
    return sb.Case(name="trainer", n=opt.n, seg_end=opt.seg_end.cpu().tolist(), seg_group=opt.seg_group.cpu().tolist(), groups=pairs,
                   p=p_before.cpu(), buf=buf_before.cpu(), grads=[opt.reducer.flat[opt.lo:opt.hi].detach().cpu().clone()],
                   momentum=opt.momentum)


def test_step_zero_meets_the_loss_and_optimizer_bounds(fx):
    tr, batch, mask, _ = fc.make_trainer(DEV, fx, fused_loss=True, flat_sgd=True)
    tr.keep_logits_grad = True
    opt = tr.optimizer
    assert len(opt.param_groups) == 62 and int(opt.seg_group.max()) == 3
    p0, b0 = opt.params.clone(), opt.momentum_buf.clone()
    r = tr.step(batch, dropout_mask=mask)
    torch.cuda.synchronize()
    bound = _xent_bound(tr, batch)
    out = torch.stack((r["loss"], r["prec1"], r["prec5"]))
    bound.check(out=out, rank=tr.criterion.rank, grad=tr.grad_logits, skipped=int(tr.criterion.skipped), what="trainer")
    # the forward before any update is float32-accurate: the reference's first loss and logits
    assert float(r["loss"]) == pytest.approx(float(fx["loss"][0]), rel=1e-4)
    assert float((tr.logits.cpu().double() - fx["logits"][0]).abs().max()) <= 1e-4 * float(fx["logits"][0].abs().max())
    assert float(r["prec1"]) == float(fx["prec1"][0]) and float(r["prec5"]) == float(fx["prec5"][0])
    case = _sgd_case(opt, p0, b0)
    assert float(case.grads[0].abs().max()) > 0
    sb.Bound(case).check(opt.params, opt.momentum_buf, 1, what="trainer")


def test_three_losses_against_the_reference(fx):
    """1e-4 relative.  Steps 2 and 3 inherit the float32 noise of the updated parameters (the step is ill-conditioned, see
    tests/test_finetune_cpu.py); the measured deviations are printed."""
    tr, batch, mask, _ = fc.make_trainer(DEV, fx)
    got = [float(tr.step(batch, dropout_mask=mask)["loss"]) for _ in range(3)]
    dev = [abs(g - float(w)) / abs(float(w)) for g, w in zip(got, fx["loss"][:3])]
    print("FINETUNE losses %s relative deviation from the reference %s" % (got, ["%.3g" % d for d in dev]))
    assert max(dev) <= 1e-4, dev


def test_the_switches_do_not_change_the_first_loss(fx):
    """The fused loss meets the bound computed from its trainer's own logits.  The composition (F.cross_entropy) adds the N logits of
    a row in float32: fewer than N more roundings on the sum, N u relative, i.e. N u absolute on the row's loss -- with the same
    SAFETY that is what it is allowed on top."""
    losses = {}
    for fused in (True, False):
        for flat in (True, False):
            tr, batch, mask, _ = fc.make_trainer(DEV, fx, fused_loss=fused, flat_sgd=flat)
            assert tr.fused_loss is fused and tr.flat_sgd is flat
            loss = float(tr.step(batch, dropout_mask=mask)["loss"])
            bound = _xent_bound(tr, batch)
            extra = 0.0 if fused else xb.SAFETY * xb.U32 * (tr.logits.shape[1] + abs(bound.out0))
            ratio = abs(loss - bound.out0) / (bound.out0_bound + extra)
            print("FINETUNE fused_loss %s flat_sgd %s: loss %.9g, error / bound %.3g" % (fused, flat, loss, ratio))
            assert ratio <= 1.0
            losses[(fused, flat)] = loss
            del tr
    assert losses[(True, True)] == losses[(True, False)] and losses[(False, True)] == losses[(False, False)]


@pytest.fixture()
def deterministic_vendor_libraries():
    """The vendor libraries' backward kernels add partial sums with atomics by default: two EAGER trainers of one seed then already
    differ in their gradients (measured: up to 1.8e-7 of a largest gradient of 0.25 after one step, with bit-equal losses).  A replay
    can only be held to an eager step bit for bit where an eager step is held to itself, so this comparison runs them in their
    deterministic modes; the project's own kernels have no such mode and need none."""
    before = (torch.backends.cudnn.deterministic, torch.are_deterministic_algorithms_enabled(),
              torch.is_deterministic_algorithms_warn_only_enabled())
    torch.backends.cudnn.deterministic = True
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = before[0]
        torch.use_deterministic_algorithms(before[1], warn_only=before[2])


def test_eager_and_replayed_steps_agree_bit_for_bit_and_the_schedule_reaches_the_replay(fx, deterministic_vendor_libraries):
    """The eager trainer runs FIRST and is done before the other one captures: the network's convolutions are the vendor library's,
    and none of them is issued eagerly beside a live graph ("one process, one captured trainer")."""
    eager, batch, mask, _ = fc.make_trainer(DEV, fx, fused_loss=True, flat_sgd=True)
    start = eager.optimizer.params.clone()
    want = []
    for step in range(4):
        if step == 3:
            eager.adjust_learning_rate(25)
        r = eager.step(batch, dropout_mask=mask)
        want.append(({k: v.clone() for k, v in r.items()}, eager.optimizer.params.clone()))
    torch.cuda.synchronize()
    del eager
    graphed, _, _, _ = fc.make_trainer(DEV, fx, fused_loss=True, flat_sgd=True, capturable=True)
    graphed.capture(batch, dropout_mask=mask)
    # the warm-up steps of capture() were real steps: back to the filled start (device copies, no network pass)
    fc.fill_network(graphed.net, float(fx["gain"]))
    graphed.optimizer.momentum_buf.zero_()
    assert torch.equal(graphed.optimizer.params, start)
    for step in range(3):
        b = graphed.step(batch, dropout_mask=mask)
        torch.cuda.synchronize()
        for k in ("loss", "prec1", "prec5"):
            assert torch.equal(want[step][0][k], b[k]), (step, k)
        assert torch.equal(want[step][1], graphed.optimizer.params), step
    # "epoch 25": the replay reads the new rates from the device tables
    opt = graphed.optimizer
    old = [g["lr"] for g in opt.param_groups]
    assert graphed.adjust_learning_rate(24) == old
    new = graphed.adjust_learning_rate(25)
    assert new == pytest.approx([v * 0.457305051927326 for v in old], rel=1e-15)
    p0, b0 = opt.params.clone(), opt.momentum_buf.clone()
    graphed.step(batch, dropout_mask=mask)
    torch.cuda.synchronize()
    case = _sgd_case(opt, p0, b0)
    assert sorted(set(g[0] for g in case.groups if g[0] > 0)) == pytest.approx(sorted(set(new)), rel=1e-15)
    sb.Bound(case).check(opt.params, opt.momentum_buf, 1, what="replay after the schedule")
    assert torch.equal(want[3][1], opt.params)
    with pytest.raises(RuntimeError):
        graphed.validate(["001"], [batch["img"][0]], batch["img"], ["001_01_01_051_07.png"] * 4)
    graphed.release_graphs()


def test_full_size_steps_with_real_dropout():
    from ffwm_amd import trainer
    tr = trainer.LightCNNTrainer(DEV, seed=1)
    assert tr.num_classes == 79077 and tr.optimizer.param_groups[0]["lr"] == 1e-4
    gen = torch.Generator().manual_seed(6)
    batch = {"img": torch.rand(10, 1, 128, 128, generator=gen).to(DEV), "target": torch.randint(0, 79077, (10,), generator=gen).to(DEV)}
    for _ in range(2):
        r = tr.step(batch)
        assert all(bool(torch.isfinite(v)) for v in r.values())
        if tr.fused_loss:
            assert int(tr.criterion.skipped) == 0
    assert bool(torch.isfinite(tr.net.fc2.weight).all()) and bool(torch.isfinite(tr.net.conv1.filter.weight).all())

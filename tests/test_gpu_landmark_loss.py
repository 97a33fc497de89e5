"""The fused landmark loss on the GPU (csrc/landmark_loss.hip): ops.landmark_loss against the per-element float64 bounds of
tests/landmark_bounds.py on every shape, scale set and family, with NaN guard cells around every gradient destination; its
run-to-run and graph-replay reproducibility; MultiScaleLDLoss / LandmarkLoss(fused=True) against float64 and the reference's
fixture; FlowNetTrainer(fused_landmarks=True) against the composed trainer, eagerly and replayed from a captured graph, and a
reverse=True step."""
import functools
import os
import sys

import pytest
import torch

import landmark_bounds as lb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import fill  # noqa: E402


@functools.lru_cache(maxsize=None)
def _case_and_bound(B, L, scales, family, dtype, seed=0):
    case = lb.make_case(B, L, scales, family, dtype, seed)
    return case, lb.Bound(case)


def _guarded(shape, dtype):
    """(NaN buffer, its middle viewed as `shape`, check()): GUARD cells before and behind the view."""
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((n + 2 * lb.GUARD,), float("nan"), dtype=dtype, device=DEV)
    view = buf[lb.GUARD:lb.GUARD + n].view(shape)

    def check():
        assert bool(torch.isnan(buf[:lb.GUARD]).all()) and bool(torch.isnan(buf[lb.GUARD + n:]).all()), "a write outside the destination"
        assert not bool(torch.isnan(view).any()), "the destination was not fully written"
    return buf, view, check


def _call(case, want_grad=True, guarded=True):
    from ffwm_amd import ops
    flows = [f.to(DEV) for f in case.flows]
    guards = [_guarded(tuple(f.shape), f.dtype) for f in flows] if guarded and want_grad else None
    out, grads, skipped = ops.landmark_loss(flows, case.lm_S.to(DEV), case.lm_F.to(DEV), case.gate.to(DEV), case.divisors, case.weights,
                                            want_grad, out_grads=None if guards is None else [g[1] for g in guards])
    torch.cuda.synchronize()
    for g in guards or []:
        g[2]()
    return out, grads, skipped


IDS = lambda sc: "/".join("%dq%d" % x for x in sc)       # noqa: E731


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("scales", lb.SCALES, ids=IDS)
@pytest.mark.parametrize("shape", lb.SHAPES, ids=lambda s: "B%dL%d" % s)
def test_entry_point_meets_the_bounds(shape, scales, dtype):
    """Every family on every shape and scale set: out, every gradient element, the cells no landmark falls on (== 0), the count of
    skipped landmarks, and the NaN guards around each gradient destination."""
    for family in lb.FAMILIES:
        case, bound = _case_and_bound(shape[0], shape[1], scales, family, dtype)
        out, grads, skipped = _call(case)
        assert out.shape == (len(scales) + 1,) and skipped.dtype == torch.int32
        bound.check(out=out, grads=grads, skipped=int(skipped), what="kernel")
        if family != "outside":
            assert int(skipped) == 0


def test_gradients_that_are_not_asked_for_are_not_written():
    """want_grad per scale: None for the others, and what is written does not depend on what was asked for."""
    case, bound = _case_and_bound(3, 67, lb.SCALES[0], "random", torch.float32)
    full = _call(case)
    some = _call(case, want_grad=(False, True, False), guarded=False)
    none = _call(case, want_grad=False)
    assert some[1][0] is None and some[1][2] is None and none[1] == [None, None, None]
    assert torch.equal(some[1][1], full[1][1])
    assert torch.equal(some[0], full[0]) and torch.equal(none[0], full[0])
    bound.check(out=none[0], what="out alone")


@pytest.mark.parametrize("spec", [(2, 1024, lb.SCALES[0], "clustered", torch.float32), (1, 1500, lb.SCALES[2], "outside", torch.float32),
                                  (3, 67, lb.SCALES[0], "random", torch.float64)], ids=lambda s: "%s-B%dL%d" % (s[3], s[0], s[1]))
def test_two_calls_agree_bit_for_bit(spec):
    case, _ = _case_and_bound(*spec)
    a, b = _call(case), _call(case, guarded=False)
    assert torch.equal(a[0], b[0]) and int(a[2]) == int(b[2])
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)


def test_a_call_replayed_from_a_graph_equals_the_eager_call():
    from ffwm_amd import ops
    case, bound = _case_and_bound(2, 1024, lb.SCALES[0], "clustered", torch.float32)
    flows = [f.to(DEV) for f in case.flows]
    lm_S, lm_F, gate = case.lm_S.to(DEV), case.lm_F.to(DEV), case.gate.to(DEV)
    eager = ops.landmark_loss(flows, lm_S, lm_F, gate, case.divisors, case.weights, True)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.landmark_loss(flows, lm_S, lm_F, gate, case.divisors, case.weights, True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, grads, skipped = ops.landmark_loss(flows, lm_S, lm_F, gate, case.divisors, case.weights, True)
    for t in [out, skipped] + grads:
        t.fill_(7)                                     # the capture executed nothing: the replays must write everything
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[0]) and int(skipped) == int(eager[2])
    for x, y in zip(grads, eager[1]):
        assert torch.equal(x, y)
    bound.check(out=out, grads=grads, skipped=int(skipped), what="replayed")


# ------------------------------------------------------------------------------------------------ the loss modules
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_fused_multi_scale_module_meets_the_bounds(dtype):
    from ffwm_amd import _lib, losses
    case, bound = _case_and_bound(2, 1024, lb.SCALES[0], "half_gated", dtype, 2)
    assert tuple(case.weights) == (1000.0, 1000.0, 1500.0)
    module = losses.MultiScaleLDLoss(fused=True)
    flows = [f.to(DEV).requires_grad_(True) for f in case.flows]
    _lib.prof_reset()
    _lib.prof_enable(True)
    loss = module(flows, case.lm_S.to(DEV), case.lm_F.to(DEV), case.gate.to(DEV))
    (loss * -0.375).backward()
    torch.cuda.synchronize()
    rows = _lib.prof_collect()
    _lib.prof_enable(False)
    assert rows["landmark_loss"]["launches"] == 1 and rows["landmark_loss_reduce"]["launches"] == 1, sorted(rows)
    assert int(module.skipped) == 0
    bound.check_module(loss.detach(), [f.grad for f in flows], grad_output=-0.375, what="MultiScaleLDLoss(fused)")
    # a flow that wants no gradient gets none; the others are unchanged
    again = [f.detach().clone().requires_grad_(i != 1) for i, f in enumerate(flows)]
    module(again, case.lm_S.to(DEV), case.lm_F.to(DEV), case.gate.to(DEV)).backward(torch.tensor(-0.375, dtype=dtype, device=DEV))
    assert again[1].grad is None and torch.equal(again[0].grad, flows[0].grad) and torch.equal(again[2].grad, flows[2].grad)


@pytest.mark.parametrize("scales", lb.SCALES[1:], ids=IDS)
def test_fused_single_scale_module_meets_the_bounds(scales):
    """LandmarkLoss divides nothing: the landmarks are those of the flow's own plane (divisor 1, weight 1)."""
    from ffwm_amd import losses
    s = scales[0][0]
    case, bound = _case_and_bound(3, 67, ((s, 1),), "outside", torch.float32, 4)
    module = losses.LandmarkLoss(fused=True)
    flow = case.flows[0].to(DEV).requires_grad_(True)
    loss = module(flow, case.lm_S.to(DEV), case.lm_F.to(DEV), case.gate.to(DEV))
    (loss * 3.5).backward()
    assert int(module.skipped) == bound.skipped > 0
    bound.check_module(loss.detach(), [flow.grad], grad_output=3.5, what="LandmarkLoss(fused)")


def test_fused_module_on_the_references_fixture():
    """The inputs of the fixture the existing composition test uses, and its tolerance."""
    from ffwm_amd import losses
    gold = torch.load(os.path.join(HERE, "golden", "reference_modules.pt"))["ld_loss"]
    flows = [fill.flow_field(2, s, s, "ld_flow%d" % s).to(DEV) for s in (128, 64, 32)]
    module = losses.MultiScaleLDLoss(fused=True)
    gate = torch.cat((gold["gate"], gold["gate"]), 2).to(DEV)
    loss = module(flows, gold["lm_S"].to(DEV), gold["lm_F"].to(DEV), gate)
    want = float(gold["loss"])
    assert abs(float(loss) - want) <= 1e-4 * (1 + abs(want)), (float(loss), want)
    assert int(module.skipped) == 0


# ------------------------------------------------------------------------------------------------ the trainer
MARGIN = 2e-3        # tests/test_gpu_sampling_correctness.py: the project's allowance for a fused loss in a trainer step


def _close(a, b):
    for k in b:
        assert abs(a[k] - b[k]) <= MARGIN * (1 + abs(b[k])), (k, a[k], b[k])


def test_flownet_step_with_the_fused_landmark_loss_matches_the_composed_step():
    from ffwm_amd import _lib, trainer
    torch.backends.cudnn.benchmark = False
    batch = trainer.synthetic_batch(2, DEV, seed=5)
    vals = []
    for fused in (True, False):
        t = trainer.FlowNetTrainer(DEV, seed=0, ngf=16, fused_landmarks=fused)
        assert t.criterionLD.fused is fused
        before = torch.cat([p.detach().flatten() for p in t.flowNet.parameters()])
        _lib.prof_reset()
        _lib.prof_enable(True)
        t.step(batch)
        torch.cuda.synchronize()
        rows = _lib.prof_collect()
        _lib.prof_enable(False)
        assert rows.get("landmark_loss", {}).get("launches", 0) == (1 if fused else 0), sorted(rows)
        v = t.loss_values()
        assert all(torch.isfinite(torch.tensor(x)) for x in v.values()), v
        after = torch.cat([p.detach().flatten() for p in t.flowNet.parameters()])
        assert float((after - before).abs().max()) > 0
        vals.append(v)
        del t
    _close(vals[0], vals[1])


def test_captured_fused_flownet_step_matches_the_eager_fused_step():
    from ffwm_amd import trainer
    torch.backends.cudnn.benchmark = False
    batch = trainer.synthetic_batch(2, DEV, seed=6)
    eager = trainer.FlowNetTrainer(DEV, seed=0, ngf=16, fused_landmarks=True)
    graphed = trainer.FlowNetTrainer(DEV, seed=0, ngf=16, fused_landmarks=True, capturable=True)
    for _ in range(2):                 # capture() runs 2 eager warm-up steps; the capture itself executes nothing
        eager.step(batch)
    graphed.capture(batch, warmup=2)
    for _ in range(3):
        eager.step(batch)
        graphed.step(batch)
    torch.cuda.synchronize()
    _close(graphed.loss_values(), eager.loss_values())
    assert int(graphed.criterionLD.skipped) == 0
    graphed.release_graphs()


def test_reverse_step_on_the_gpu():
    from ffwm_amd import trainer
    torch.backends.cudnn.benchmark = False
    batch = trainer.synthetic_batch(2, DEV, seed=7)
    t = trainer.FlowNetTrainer(DEV, seed=0, ngf=16, reverse=True, fused_landmarks=True)
    before = torch.cat([p.detach().flatten() for p in t.flowNet.parameters()])
    t.step(batch)
    torch.cuda.synchronize()
    v = t.loss_values()
    assert set(v) == {"loss", "cor", "reg", "lm"} and all(torch.isfinite(torch.tensor(x)) for x in v.values()), v
    after = torch.cat([p.detach().flatten() for p in t.flowNet.parameters()])
    assert float((after - before).abs().max()) > 0 and bool(torch.isfinite(after).all())

"""The fused sampling-correctness loss on the GPU: the entry point against the per-pixel float64 bounds of
tests/correctness_bounds.py through the C ABI (every shape, family and mask of its matrix), its NULL outputs and its run-to-run
reproducibility; PerceptualCorrectness(fused=True) against the composition; FlowNetTrainer(fused_correctness=True) against the
composed trainer, eagerly and replayed from a captured graph."""
import functools

import pytest
import torch

import correctness_bounds as cb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SPECS = cb.cases()


@functools.lru_cache(maxsize=None)
def _case_and_bound(spec):
    case = cb.build(spec)
    return case, cb.Bound(case)


def _guarded(n, dtype):
    return torch.full((n + cb.GUARD,), float("nan"), dtype=dtype, device=DEV)


def _guards_intact(buf, n):
    return bool(torch.isnan(buf[n:]).all())


def _call(case, want_map=True, want_grad=True):
    """One call through the C ABI -> (out[2], loss_map or None, grad_flow or None), every output with NaN guard cells behind it."""
    from ffwm_amd import _lib
    lib = _lib.load()
    B, C, Hi, Wi, H, W = case.dims
    dt = case.source.dtype
    code = _lib.F32 if dt == torch.float32 else _lib.F64
    dev = [None if t is None else t.to(DEV) for t in (case.source, case.target, case.flow, case.corr_max, case.mask)]
    nbytes = lib.ffwm_sampling_correctness_workspace_bytes(B, H, W, code)
    assert nbytes > 0
    ws = _guarded(nbytes // 8, torch.float64)
    out = _guarded(2, dt)
    lmap = _guarded(B * H * W, dt) if want_map else None
    grad = _guarded(2 * B * H * W, dt) if want_grad else None
    ptr = [None if t is None else t.data_ptr() for t in dev + [lmap, grad, out, ws]]
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.ffwm_sampling_correctness(*ptr, B, C, Hi, Wi, H, W, case.e1, case.eps, code, stream), "ffwm_sampling_correctness")
    torch.cuda.synchronize()
    assert _guards_intact(ws, nbytes // 8) and _guards_intact(out, 2)
    assert lmap is None or _guards_intact(lmap, B * H * W)
    assert grad is None or _guards_intact(grad, 2 * B * H * W)
    return (out[:2], None if lmap is None else lmap[:B * H * W].view(B, H * W),
            None if grad is None else grad[:2 * B * H * W].view(B, 2, H, W))


@pytest.mark.parametrize("i", range(len(SPECS)), ids=[cb.case_id(s) for s in SPECS])
def test_entry_point_meets_the_bounds(i):
    """Every case of the matrix; the loss map is asked for in every other one (the gradient and out always)."""
    case, bound = _case_and_bound(SPECS[i])
    out, lmap, grad = _call(case, want_map=i % 2 == 0)
    assert (lmap is None) == (i % 2 == 1)
    bound.check(out=out, loss_map=lmap, grad_flow=grad, what="kernel ls=%d" % cb.lane_slices(case.dims))


@pytest.mark.parametrize("spec", [("c70_ragged", "mixed", "binary"), ("c3", "left", "none")], ids=cb.case_id)
def test_null_outputs_are_skipped_and_the_rest_is_unchanged(spec):
    """grad_flow NULL and loss_map NULL: a NaN-filled buffer that is NOT handed over stays NaN, and what is written does not depend
    on which outputs were asked for."""
    case, bound = _case_and_bound(spec)
    B, C, Hi, Wi, H, W = case.dims
    bystander = torch.full((2 * B * H * W + cb.GUARD,), float("nan"), dtype=case.source.dtype, device=DEV)
    full = _call(case, True, True)
    only_map = _call(case, True, False)
    only_grad = _call(case, False, True)
    neither = _call(case, False, False)
    torch.cuda.synchronize()
    assert bool(torch.isnan(bystander).all())
    assert only_map[2] is None and only_grad[1] is None and neither[1] is None and neither[2] is None
    for other in (only_map, only_grad, neither):
        assert torch.equal(other[0], full[0])
    assert torch.equal(only_map[1], full[1]) and torch.equal(only_grad[2], full[2])
    bound.check(out=neither[0], what="out alone")


@pytest.mark.parametrize("spec", [("c256", "random", "binary"), ("c32_1024_blocks", "mixed", "binary"), ("c5_f64", "mixed", "none")],
                         ids=cb.case_id)
def test_two_calls_agree_bit_for_bit(spec):
    case, _ = _case_and_bound(spec)
    a, b = _call(case), _call(case)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ the loss module
def _module_case(spec):
    """The case with the correlation maximum the module forms on the GPU (the same torch ops, so the same values)."""
    case = cb.build(spec, seed=3)
    case.corr_max = cb.correlation_max(case.source.to(DEV), case.target.to(DEV), case.eps).cpu()
    return case


def _module_run(case, fused, source_grad=False):
    from ffwm_amd import external_function, losses
    B, C, Hi, Wi, H, W = case.dims
    pc = losses.PerceptualCorrectness(None, external_function.WarpNet(), fused=fused)
    source = case.source.to(DEV).requires_grad_(source_grad)
    pc.target_vgg, pc.source_vgg = {"x": case.target.to(DEV)}, {"x": source}
    flow = case.flow.to(DEV).requires_grad_(True)
    mask = None if case.mask is None else case.mask.to(DEV).reshape(B, 1, H, W)
    loss = pc.calculate_loss(flow, "x", mask, use_bilinear_sampling=True)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), flow.grad.cpu(), source.grad


@pytest.mark.parametrize("spec", [("c64", "smooth", "binary"), ("c70_ragged", "bottom", "none"), ("c3", "mixed", "binary"),
                                  ("c5_f64", "random", "binary")], ids=cb.case_id)
def test_fused_module_matches_the_composition(spec):
    """Both paths meet the bounds of the float64 reference, so they agree within the sum of their bounds (asserted as such)."""
    from ffwm_amd import _lib
    case = _module_case(spec)
    fused_bound, composed_bound = cb.Bound(case), cb.Bound(case, float_sums=True)
    _lib.prof_reset()
    _lib.prof_enable(True)
    lf, gf, _ = _module_run(case, True)
    rows = _lib.prof_collect()
    _lib.prof_enable(False)
    assert rows["sampling_correctness"]["launches"] == 1 and not any(k.startswith("warp") for k in rows), sorted(rows)
    lc, gc, _ = _module_run(case, False)
    fused_bound.check_module(lf, gf, what="fused module")
    composed_bound.check_module(lc, gc, what="composed module")
    assert abs(float(lf) - float(lc)) <= fused_bound.out_bound + composed_bound.out_bound
    per_pixel = (fused_bound.grad_bound + composed_bound.grad_bound) / fused_bound.ref_out1 \
        + 4 * fused_bound.twice * fused_bound.U * (fused_bound.ref_grad / fused_bound.ref_out1).abs()
    assert bool(((gf.double() - gc.double()).abs() <= per_pixel + cb.FLOOR).all())


def test_source_features_that_want_a_gradient_take_the_composition():
    from ffwm_amd import _lib
    case = _module_case(("c64", "random", "binary"))
    _lib.prof_reset()
    _lib.prof_enable(True)
    loss, grad, source_grad = _module_run(case, True, source_grad=True)
    rows = _lib.prof_collect()
    _lib.prof_enable(False)
    assert "sampling_correctness" not in rows and any(k.startswith("warp") for k in rows), sorted(rows)
    assert source_grad is not None and bool(torch.isfinite(source_grad).all()) and float(source_grad.abs().max()) > 0
    cb.Bound(case, float_sums=True).check_module(loss, grad, what="composition (source wants a gradient)")


def test_empty_grid_launches_nothing_and_returns_the_compositions_value():
    from ffwm_amd import ops
    z = lambda *s: torch.zeros(*s, device=DEV)
    out, grad, _ = ops.sampling_correctness(z(0, 4, 5, 5), z(0, 4, 3, 3), z(0, 2, 3, 3), z(0, 9), z(0, 9), 1e-8, True)
    want = (torch.sum(z(0, 9)) - cb.exp_minus_one(torch.float32)) / (torch.sum(z(0, 9)) + 1e-8)
    assert float(out[0]) == float(want) and grad.shape == (0, 2, 3, 3)
    out, _, _ = ops.sampling_correctness(z(0, 4, 5, 5), z(0, 4, 3, 3), z(0, 2, 3, 3), z(0, 9), None, 1e-8, False)
    assert bool(torch.isnan(out[0])) and bool(torch.isnan(torch.mean(z(0, 9)) - 0.5))


# ------------------------------------------------------------------------------------------------ the trainer
MARGIN = 2e-3        # what test_flownet_pretraining_step_on_gpu_fused_vs_composed_regulariser grants a fused loss


def _close(a, b):
    for k in b:
        assert abs(a[k] - b[k]) <= MARGIN * (1 + abs(b[k])), (k, a[k], b[k])


def test_flownet_step_with_the_fused_correctness_loss_matches_the_composed_step():
    from ffwm_amd import _lib, trainer
    torch.backends.cudnn.benchmark = False
    batch = trainer.synthetic_batch(2, DEV, seed=5)
    vals = []
    for fused in (True, False):
        t = trainer.FlowNetTrainer(DEV, seed=0, ngf=16, fused_correctness=fused)
        assert t.Correctness.fused is fused
        before = torch.cat([p.detach().flatten() for p in t.flowNet.parameters()])
        _lib.prof_reset()
        _lib.prof_enable(True)
        t.step(batch)
        torch.cuda.synchronize()
        rows = _lib.prof_collect()
        _lib.prof_enable(False)
        assert rows.get("sampling_correctness", {}).get("launches", 0) == (3 if fused else 0), sorted(rows)
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
    eager = trainer.FlowNetTrainer(DEV, seed=0, ngf=16, fused_correctness=True)
    graphed = trainer.FlowNetTrainer(DEV, seed=0, ngf=16, fused_correctness=True, capturable=True)
    for _ in range(2):                 # capture() runs 2 eager warm-up steps; the capture itself executes nothing
        eager.step(batch)
    graphed.capture(batch, warmup=2)
    for _ in range(3):
        eager.step(batch)
        graphed.step(batch)
    torch.cuda.synchronize()
    _close(graphed.loss_values(), eager.loss_values())
    graphed.release_graphs()

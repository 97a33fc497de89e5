"""CPU side of the fused landmark loss (csrc/landmark_loss.hip): the bounds of tests/landmark_bounds.py against a float32 emulation
of the kernel's arithmetic, the C entry point's argument checks (they come before any launch), the wrappers' refusals, and that
every new option is off by default and changes nothing on CPU tensors."""
import ctypes
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import landmark_bounds as lb  # noqa: E402


@pytest.mark.parametrize("scales", lb.SCALES, ids=lambda sc: "/".join("%dq%d" % x for x in sc))
@pytest.mark.parametrize("shape", lb.SHAPES, ids=lambda s: "B%dL%d" % s)
def test_float32_emulation_meets_a_quarter_of_the_bounds(shape, scales):
    """SAFETY = 4 multiplies every count of roundings: arithmetic that rounds as often as the kernel does, in another order of the
    additions, stays within a quarter of the allowance -- on every family."""
    for family in lb.FAMILIES:
        case = lb.make_case(shape[0], shape[1], scales, family)
        bound = lb.Bound(case)
        out, grads, skipped = lb.emulate(case)
        bound.check(out=out, grads=grads, skipped=skipped, what="emulation", factor=0.25)


def test_the_bounds_notice_a_wrong_result():
    """A bound that anything meets shows nothing: one ulp-scale slip per check must fail it."""
    case = lb.make_case(2, 40, lb.SCALES[0], "random")
    bound = lb.Bound(case)
    out, grads, skipped = lb.emulate(case)
    sc = bound.scales[1]
    b, c, y, x = [int(v[0]) for v in torch.nonzero(sc.touched, as_tuple=True)]
    wrong = [g.clone() for g in grads]
    wrong[1][b, c, y, x] *= 1 + 2e-4
    with pytest.raises(AssertionError):
        bound.check(grads=wrong, verbose=False)
    wrong = [g.clone() for g in grads]
    wrong[2][~bound.scales[2].touched] = 1e-30                     # a cell no landmark falls on must be exactly 0
    with pytest.raises(AssertionError):
        bound.check(grads=wrong, verbose=False)
    with pytest.raises(AssertionError):
        bound.check(out=out * (1 + 1e-5), verbose=False)
    with pytest.raises(AssertionError):
        bound.check(skipped=skipped + 1, verbose=False)
    # the reference is the module's own composition in float64
    from ffwm_amd import losses
    flows = [f.double().requires_grad_(True) for f in case.flows]
    loss = losses.MultiScaleLDLoss()(flows, case.lm_S, case.lm_F, case.gate.double())
    loss.backward()
    assert abs(float(loss.detach()) - bound.out0) <= 1e-12 * abs(bound.out0)
    for f, sc in zip(flows, bound.scales):
        assert float((f.grad - sc.grad).abs().max()) <= 1e-12 * float(sc.grad.abs().max())


def test_new_options_are_off_by_default():
    from ffwm_amd import losses, trainer
    assert inspect.signature(losses.LandmarkLoss.__init__).parameters["fused"].default is False
    assert inspect.signature(losses.MultiScaleLDLoss.__init__).parameters["fused"].default is False
    params = inspect.signature(trainer.FlowNetTrainer.__init__).parameters
    assert params["fused_landmarks"].default is False and params["reverse"].default is False


def test_fused_modules_on_cpu_tensors_run_the_composition_unchanged():
    from ffwm_amd import losses
    case = lb.make_case(2, 67, lb.SCALES[0], "random", seed=1)
    results = []
    for fused in (False, True):
        flows = [f.clone().requires_grad_(True) for f in case.flows]
        module = losses.MultiScaleLDLoss(fused=True) if fused else losses.MultiScaleLDLoss()
        loss = module(flows, case.lm_S, case.lm_F, case.gate)
        (loss * 0.75).backward()
        results.append((loss.detach(), [f.grad for f in flows]))
        assert module.skipped is None
    assert torch.equal(results[0][0], results[1][0])
    assert all(torch.equal(a, b) for a, b in zip(results[0][1], results[1][1]))
    one = [case.flows[0].clone().requires_grad_(True) for _ in range(2)]
    la = losses.LandmarkLoss()(one[0], case.lm_S, case.lm_F, case.gate)
    lb_ = losses.LandmarkLoss(fused=True)(one[1], case.lm_S, case.lm_F, case.gate)
    la.backward()
    lb_.backward()
    assert torch.equal(la.detach(), lb_.detach()) and torch.equal(one[0].grad, one[1].grad)


def test_wrapper_refuses_cpu_tensors_and_bad_shapes():
    from ffwm_amd import ops
    case = lb.make_case(2, 5, lb.SCALES[0], "random")
    args = (case.lm_S, case.lm_F, case.gate, case.divisors, case.weights, True)
    with pytest.raises(NotImplementedError):
        ops.landmark_loss(case.flows, *args)
    with pytest.raises(ValueError):
        ops.landmark_loss([torch.zeros(2, 2, 8, 9)], case.lm_S, case.lm_F, case.gate, [1], [1.0], True)          # not square
    with pytest.raises(ValueError):
        ops.landmark_loss([torch.zeros(0, 2, 8, 8)], case.lm_S[:0], case.lm_F[:0], case.gate[:0], [1], [1.0], True)   # B == 0
    with pytest.raises(ValueError):
        ops.landmark_loss(case.flows, case.lm_S[:, :0], case.lm_F[:, :0], case.gate[:, :0], case.divisors, case.weights, True)   # L == 0
    with pytest.raises(ValueError):
        ops.landmark_loss(case.flows, case.lm_S, case.lm_F[:, :4], case.gate, case.divisors, case.weights, True)  # mismatched
    with pytest.raises(ValueError):
        ops.landmark_loss(case.flows, case.lm_S, case.lm_F, case.gate, case.divisors[:2], case.weights, True)
    with pytest.raises(ValueError):
        ops.landmark_loss(case.flows * 2, case.lm_S, case.lm_F, case.gate, case.divisors * 2, case.weights * 2, True)   # 6 scales
    with pytest.raises(ValueError):
        ops.landmark_loss(case.flows, case.lm_S, case.lm_F, case.gate, [1, 0, 4], case.weights, True)


def test_entry_point_checks_its_arguments_before_any_launch():
    from ffwm_amd import _lib, build
    build.build()
    lib = _lib.load()
    for name in ("ffwm_landmark_loss", "ffwm_landmark_loss_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert lib.ffwm_abi_version() == 5
    assert lib.ffwm_set_option(b"landmark_loss", 1) == -1                       # no tuning key came with it
    i64 = ctypes.c_int64
    sides = (i64 * 3)(128, 64, 32)
    ws = lib.ffwm_landmark_loss_workspace_bytes
    assert ws.restype is ctypes.c_int64
    assert ws(sides, 3, 6, 1024, _lib.F32) == 16 * 6 * (64 + 16 + 4)          # two doubles per 256-cell block
    assert ws((i64 * 1)(20), 1, 1, 1, _lib.F64) == 16 * 2
    assert ws(sides, 0, 6, 1024, _lib.F32) == -1 and ws(sides, 5, 6, 1024, _lib.F32) == -1
    assert ws(sides, 3, 0, 1024, _lib.F32) == -1 and ws(sides, 3, 6, 0, _lib.F32) == -1
    assert ws(sides, 3, 6, 1024, 7) == -2
    assert ws((i64 * 1)(5000), 1, 1, 1, _lib.F32) == -3 and ws(sides, 3, 1 << 31, 4, _lib.F32) == -3
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    flows = (ctypes.c_void_p * 4)(p.value, p.value, p.value, p.value)
    div = (i64 * 3)(1, 2, 4)
    wts = (ctypes.c_double * 3)(1000.0, 1000.0, 1500.0)
    fn = lib.ffwm_landmark_loss

    def call(flows=flows, grads=None, sides=sides, div=div, wts=wts, n=3, lm_S=p, lm_F=p, gate=p, out=p, skipped=p, wsp=p, B=2, L=5,
             dtype=_lib.F32):
        return fn(flows, grads, sides, div, wts, n, lm_S, lm_F, gate, out, skipped, wsp, B, L, dtype, None)

    assert call(lm_S=None) == -1 and b"NULL" in lib.ffwm_last_error()
    assert call(flows=None) == -1 and call(out=None) == -1 and call(skipped=None) == -1 and call(gate=None) == -1
    assert call(wsp=None) == -1 and b"workspace" in lib.ffwm_last_error()
    assert call(wsp=ctypes.c_void_p(p.value + 4)) == -1 and b"aligned" in lib.ffwm_last_error()
    assert call(flows=(ctypes.c_void_p * 4)(p.value, None, p.value, p.value)) == -1 and b"scale 1" in lib.ffwm_last_error()
    assert call(n=0) == -1 and call(n=5) == -1 and b"n_scales" in lib.ffwm_last_error()
    assert call(dtype=3) == -2
    assert call(B=0) == -1 and call(L=0) == -1
    assert call(div=(i64 * 3)(1, 0, 4)) == -1 and b"divisor" in lib.ffwm_last_error()
    assert call(sides=(i64 * 3)(128, 0, 32)) == -1
    assert call(sides=(i64 * 3)(128, 4097, 32)) == -3
    assert call(div=(i64 * 3)(1, 1 << 31, 4)) == -3
    assert call(L=(1 << 30) + 1) == -3

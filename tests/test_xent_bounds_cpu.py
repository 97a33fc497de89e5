"""CPU side of the fused classifier loss (csrc/softmax_xent.hip): the bounds of tests/xent_bounds.py against a float32 emulation of
the kernel's arithmetic, a deliberately wrong emulation that must violate them, the C entry point's argument checks (they come before
any launch), and ClassifierLoss's composition on CPU tensors."""
import ctypes
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xent_bounds as xb  # noqa: E402


@pytest.fixture(scope="module")
def hiplib():
    from ffwm_amd import build, _lib
    build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def chunk(hiplib):
    c = hiplib.ffwm_softmax_xent_chunk()
    assert c >= 64 and c % 4 == 0
    return c


@pytest.mark.parametrize("family", xb.FAMILIES)
def test_float32_emulation_meets_the_bounds(family, chunk):
    """Arithmetic that rounds as often as the kernel does stays inside the allowance on every family and shape."""
    for B, N in xb.shapes(chunk):
        case = xb.make_case(B, N, family)
        out, row_loss, rank, grad, skipped = xb.emulate(case, chunk)
        xb.Bound(case, chunk).check(out=out, row_loss=row_loss, rank=rank, grad=grad, skipped=skipped, what="emulation")


def test_float64_emulation_meets_the_bounds(chunk):
    for family in xb.FAMILIES:
        case = xb.make_case(3, 257, family, torch.float64)
        out, row_loss, rank, grad, skipped = xb.emulate(case, chunk)
        xb.Bound(case, chunk).check(out=out, row_loss=row_loss, rank=rank, grad=grad, skipped=skipped, what="emulation")


def test_the_bounds_notice_a_missing_max_subtraction(chunk):
    """exp(80) = 5.5e34 still fits float32, so the `wide` family alone does not overflow an exp of the raw logits; softmax does not change
    when every logit moves by the same amount, and 100 higher the raw exp overflows: the wrong emulation's loss is then not finite."""
    case = xb.make_case(3, 257, "wide")
    case.logits = (case.logits.double() + 100).float()
    bound = xb.Bound(case, chunk)
    out, row_loss, rank, grad, skipped = xb.emulate(case, chunk)
    bound.check(out=out, row_loss=row_loss, rank=rank, grad=grad, skipped=skipped, what="emulation")
    out, row_loss, rank, grad, skipped = xb.emulate(case, chunk, subtract_max=False)
    with pytest.raises(AssertionError):
        bound.check(out=out, verbose=False)
    with pytest.raises(AssertionError):
        bound.check(row_loss=row_loss, verbose=False)
    with pytest.raises(AssertionError):
        bound.check(grad=grad, verbose=False)


def test_the_bounds_notice_a_wrong_result(chunk):
    """A bound that anything meets shows nothing: one slip per check must fail it."""
    case = xb.make_case(3, 257, "random")
    bound = xb.Bound(case, chunk)
    out, row_loss, rank, grad, skipped = xb.emulate(case, chunk)
    wrong = grad.clone()
    wrong[1, 7] *= 1 + 1e-4
    with pytest.raises(AssertionError):
        bound.check(grad=wrong, verbose=False)
    with pytest.raises(AssertionError):
        bound.check(out=out * (1 + 1e-5), verbose=False)
    with pytest.raises(AssertionError):
        bound.check(rank=rank + 1, verbose=False)
    with pytest.raises(AssertionError):
        bound.check(skipped=skipped + 1, verbose=False)
    masked = xb.make_case(3, 257, "masked")
    mb = xb.Bound(masked, chunk)
    g = xb.emulate(masked, chunk)[3]
    g[masked.logits == -math.inf] = 1e-30                     # a -inf logit's gradient must be exactly 0
    with pytest.raises(AssertionError):
        mb.check(grad=g, verbose=False)
    # the reference is the module's own composition in float64
    from ffwm_amd import losses
    x = case.logits.double().requires_grad_(True)
    crit = losses.ClassifierLoss()
    loss = crit(x, case.target)
    loss.backward()
    assert abs(float(loss.detach()) - bound.out0) <= 1e-12 * abs(bound.out0)
    assert float((x.grad - bound.grad).abs().max()) <= 1e-12 * float(bound.grad.abs().max())
    assert [float(crit.prec1), float(crit.prec5)] == pytest.approx(bound.prec, rel=1e-6)
    assert xb.reference_accuracy(case.logits, case.target) == pytest.approx(bound.prec, rel=1e-6)


def test_classifier_loss_falls_back_on_cpu_tensors():
    from ffwm_amd import losses
    case = xb.make_case(2, 5, "random")
    crit = losses.ClassifierLoss(fused=True)
    loss = crit(case.logits, case.target)
    assert float(loss) == pytest.approx(float(torch.nn.functional.cross_entropy(case.logits, case.target)))
    assert crit.prec1.shape == () and crit.prec5.shape == () and float(crit.prec5) == 100.0
    from ffwm_amd import ops
    with pytest.raises(NotImplementedError):
        ops.softmax_xent(case.logits, case.target)


def test_argument_errors_are_reported_before_launch(hiplib):
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = hiplib.ffwm_softmax_xent
    assert call(None, p, p, p, p, p, p, p, 2, 5, 0, None) == -1 and b"NULL" in hiplib.ffwm_last_error()
    assert call(p, None, p, p, p, p, p, p, 2, 5, 0, None) == -1
    assert call(p, p, None, p, p, p, p, p, 2, 5, 0, None) == -1
    assert call(p, p, p, p, p, p, None, p, 2, 5, 0, None) == -1 and b"skipped" in hiplib.ffwm_last_error()
    assert call(p, p, p, p, p, p, p, None, 2, 5, 0, None) == -1 and b"workspace" in hiplib.ffwm_last_error()
    assert call(p, p, p, p, p, p, p, p, 0, 5, 0, None) == -1
    assert call(p, p, p, p, p, p, p, p, 2, 0, 0, None) == -1
    assert call(p, p, p, p, p, p, p, p, 2, (1 << 24) + 1, 0, None) == -3 and b"2^24" in hiplib.ffwm_last_error()
    assert call(p, p, p, p, p, p, p, p, 2, 5, 7, None) == -2 and b"dtype" in hiplib.ffwm_last_error()
    size = hiplib.ffwm_softmax_xent_workspace_bytes
    assert size(2, 5, 7) == -2 and size(0, 5, 0) == -1 and size(2, (1 << 24) + 1, 0) == -3
    c = hiplib.ffwm_softmax_xent_chunk()
    assert size(10, 79077, 0) == size(10, 79077, 1) >= 10 * ((79077 + c - 1) // c) * 24 and size(10, 79077, 0) % 8 == 0


def test_header_exports_and_binding_agree(hiplib):
    from ffwm_amd import _lib
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ffwm_hip.h")).read()
    for name in ("ffwm_softmax_xent", "ffwm_softmax_xent_chunk", "ffwm_softmax_xent_workspace_bytes"):
        assert name + "(" in text and name in _lib.EXPORTS and hasattr(hiplib, name)
    assert hiplib.ffwm_abi_version() == 5

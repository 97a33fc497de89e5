"""CPU side of the flat SGD step (csrc/sgd.hip): the bounds of tests/sgd_bounds.py against a float32 emulation of the kernel's
arithmetic and against torch.optim.SGD itself, a deliberately wrong emulation that must violate them, and the C entry point's
argument checks (they come before any launch)."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgd_bounds as sb  # noqa: E402

CASES = sb.cases()


@pytest.fixture(scope="module")
def hiplib():
    from ffwm_amd import build, _lib
    build.build()
    return _lib.load()


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_float32_emulation_meets_the_bounds(case):
    bound = sb.Bound(case)
    for steps in (1, 3):
        p, buf = sb.emulate(case, steps)
        bound.check(p, buf, steps, what="emulation")


@pytest.mark.parametrize("case", CASES[:6], ids=repr)
def test_the_reference_is_torch_sgd(case):
    """The float64 recurrence of sgd_bounds.Bound is torch.optim.SGD's: one group per segment, as lightcnn/finetune.py builds them,
    from a zero buffer (torch creates it on the first step)."""
    zero = sb.Case(**dict(case.__dict__, buf=torch.zeros_like(case.buf)))
    bound = sb.Bound(zero)
    params, a = [], 0
    for e in case.seg_end:
        params.append(torch.nn.Parameter(case.p[a:e].double().clone()))
        a = e
    opt = torch.optim.SGD([{"params": [q], "lr": case.groups[k][0], "weight_decay": case.groups[k][1]}
                           for q, k in zip(params, case.seg_group)], lr=1.0, momentum=case.momentum)
    for g in case.grads:
        a = 0
        for q, e in zip(params, case.seg_end):
            q.grad = g[a:e].double().clone()
            a = e
        opt.step()
    got = torch.cat([q.detach() for q in params])
    assert float((got - bound.p[3]).abs().max()) <= 1e-14 * max(1.0, float(got.abs().max()))


def test_the_bounds_notice_weight_decay_on_a_group_without_one():
    case = CASES[4]
    bound = sb.Bound(case)
    p, buf = sb.emulate(case, 1, decay_everywhere=True)
    with pytest.raises(AssertionError):
        bound.check(p, buf, 1, verbose=False)
    p, buf = sb.emulate(case, 1)
    moved = p.clone()
    frozen = torch.nonzero(bound.lr == 0)[0]
    moved[frozen] = torch.nextafter(moved[frozen], torch.tensor(2.0))          # a parameter of the frozen group: any change fails
    with pytest.raises(AssertionError):
        bound.check(moved, buf, 1, verbose=False)
    with pytest.raises(AssertionError):
        bound.check(p, buf * (1 + 1e-5), 1, verbose=False)


def test_argument_errors_are_reported_before_launch(hiplib):
    raw = (ctypes.c_double * 64)()
    base = ctypes.addressof(raw)
    p = ctypes.c_void_p((base + 15) // 16 * 16)
    odd = ctypes.c_void_p(p.value + 4)
    call = hiplib.ffwm_sgd_step
    ok = [p, p, p, 8, p, p, 1, p, p, 1, 0.9, 0, None]

    def with_(i, v):
        a = list(ok)
        a[i] = v
        return call(*a)
    for i in (0, 1, 2, 4, 5, 7, 8):
        assert with_(i, None) == -1 and b"NULL" in hiplib.ffwm_last_error(), i
    assert with_(3, 0) == -1
    assert with_(6, 0) == -1 and with_(6, 1025) == -1 and b"n_seg" in hiplib.ffwm_last_error()
    assert with_(9, 0) == -1 and with_(9, 17) == -1 and b"n_groups" in hiplib.ffwm_last_error()
    assert with_(11, 1) == -2 and b"float32" in hiplib.ffwm_last_error()
    assert with_(0, odd) == -1 and b"aligned" in hiplib.ffwm_last_error()


def test_header_exports_and_binding_agree(hiplib):
    from ffwm_amd import _lib
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ffwm_hip.h")).read()
    assert "ffwm_sgd_step(" in text and "ffwm_sgd_step" in _lib.EXPORTS and hasattr(hiplib, "ffwm_sgd_step")
    assert hiplib.ffwm_abi_version() == 5

"""The fused classifier loss on the GPU (csrc/softmax_xent.hip): ops.softmax_xent against the per-element float64 bounds of
tests/xent_bounds.py on every shape, family and dtype, with NaN guard cells around grad_logits and row_loss; want_grad=False; its
run-to-run and graph-replay reproducibility; ClassifierLoss(fused=True) through autograd against float64; prec@1 / prec@5 against
the reference's accuracy() restated with topk."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xent_bounds as xb  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _chunk():
    from ffwm_amd import ops
    return ops.softmax_xent_chunk()


@functools.lru_cache(maxsize=None)
def _case_and_bound(B, N, family, dtype, seed=0):
    case = xb.make_case(B, N, family, dtype, seed)
    return case, xb.Bound(case, _chunk())


def _guarded(shape, dtype):
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((n + 2 * xb.GUARD,), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[xb.GUARD:xb.GUARD + n].view(shape)


def _guards_intact(buf):
    return bool(torch.isnan(buf[:xb.GUARD]).all()) and bool(torch.isnan(buf[buf.numel() - xb.GUARD:]).all())


def _call(case, want_grad=True):
    """The C entry point with guarded destinations for grad_logits and row_loss -> (out, row_loss, rank, grad, skipped)."""
    from ffwm_amd import _lib, ops
    x, t = case.logits.to(DEV), case.target.to(DEV)
    B, N = x.shape
    code = ops._dtype_code(x)
    lib = _lib.load()
    gbuf, grad = _guarded((B, N), x.dtype)
    lbuf, row_loss = _guarded((B,), x.dtype)
    out = x.new_empty(3)
    rank = torch.empty(B, dtype=torch.int32, device=DEV)
    skipped = torch.empty((), dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.ffwm_softmax_xent_workspace_bytes(B, N, code) // 8, dtype=torch.float64, device=DEV)
    with ops._on_device(x) as stream:
        _lib.check(lib.ffwm_softmax_xent(x.data_ptr(), t.data_ptr(), out.data_ptr(), row_loss.data_ptr(), rank.data_ptr(),
                                         grad.data_ptr() if want_grad else None, skipped.data_ptr(), ws.data_ptr(), B, N, code, stream),
                   "ffwm_softmax_xent")
    torch.cuda.synchronize()
    assert _guards_intact(gbuf) and _guards_intact(lbuf), "a write outside a destination"
    if not want_grad:
        assert bool(torch.isnan(grad).all()), "a gradient was written although none was asked for"
        grad = None
    return out, row_loss, rank, grad, skipped


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("family", xb.FAMILIES)
def test_entry_point_meets_the_bounds(family, dtype):
    """Every shape on every family: out, every row's loss and rank, every gradient element (== 0 at -inf logits and in skipped rows),
    the count of skipped rows, and the NaN guards around both destinations."""
    for B, N in xb.shapes(_chunk()):
        case, bound = _case_and_bound(B, N, family, dtype)
        out, row_loss, rank, grad, skipped = _call(case)
        assert out.shape == (3,) and skipped.dtype == torch.int32 and rank.dtype == torch.int32
        if family not in ("nan_row",):
            assert not bool(torch.isnan(grad).any()), "the gradient was not fully written"
        bound.check(out=out, row_loss=row_loss, rank=rank, grad=grad, skipped=int(skipped), what="kernel")
        if family != "outside":
            assert int(skipped) == 0


@pytest.mark.parametrize("shape", [(3, 257), (10, 79077)], ids=lambda s: "B%dN%d" % s)
def test_without_a_gradient_the_rest_is_bit_equal(shape):
    case, bound = _case_and_bound(shape[0], shape[1], "random", torch.float32)
    full, bare = _call(case), _call(case, want_grad=False)
    assert bare[3] is None
    for a, b in zip(full[:3] + full[4:], bare[:3] + bare[4:]):
        assert torch.equal(a, b)
    bound.check(out=bare[0], row_loss=bare[1], rank=bare[2], skipped=int(bare[4]), what="no gradient")


def test_the_python_wrapper_without_a_gradient_and_with_a_destination():
    """ops.softmax_xent(want_grad=False) returns no gradient and the rest bit-equal; out_grad= is the destination that is written
    (and returned), with its NaN guards intact; a destination of another shape or dtype is refused.  ClassifierLoss(fused=True) on
    logits that need no gradient takes the kernel's no-gradient branch."""
    from ffwm_amd import losses, ops
    case, bound = _case_and_bound(2, _chunk() + 1, "masked", torch.float32)
    x, t = case.logits.to(DEV), case.target.to(DEV)
    full = ops.softmax_xent(x, t)
    bare = ops.softmax_xent(x, t, want_grad=False)
    assert bare[3] is None and full[3] is not None
    for a, b in zip(full[:3] + full[4:], bare[:3] + bare[4:]):
        assert torch.equal(a, b)
    gbuf, dest = _guarded(tuple(x.shape), x.dtype)
    given = ops.softmax_xent(x, t, out_grad=dest)
    torch.cuda.synchronize()
    assert given[3] is dest and _guards_intact(gbuf) and torch.equal(dest, full[3])
    bound.check(out=given[0], row_loss=given[1], rank=given[2], grad=dest, skipped=int(given[4]), what="out_grad")
    with pytest.raises(ValueError):
        ops.softmax_xent(x, t, out_grad=torch.empty(2, 3, device=DEV))
    with pytest.raises(ValueError):
        ops.softmax_xent(x, t, out_grad=torch.empty_like(x, dtype=torch.float64))
    crit = losses.ClassifierLoss(fused=True)
    loss = crit(x, t)                                   # requires_grad is False: no gradient is computed or kept
    assert not loss.requires_grad and torch.equal(loss, full[0][0]) and torch.equal(crit.rank, full[2])
    assert torch.equal(crit.prec1, full[0][1]) and torch.equal(crit.prec5, full[0][2]) and int(crit.skipped) == 0
    with torch.no_grad():
        assert torch.equal(crit(x.clone().requires_grad_(True), t), full[0][0])


@pytest.mark.parametrize("spec", [(10, 79077, "random", torch.float32), (3, 257, "wide", torch.float64), (2, 5, "outside", torch.float32)],
                         ids=lambda s: "%s-B%dN%d" % (s[2], s[0], s[1]))
def test_two_calls_and_a_graph_replay_agree_bit_for_bit(spec):
    from ffwm_amd import ops
    case, _ = _case_and_bound(*spec)
    a, b = _call(case), _call(case)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    x, t = case.logits.to(DEV), case.target.to(DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        ops.softmax_xent(x, t)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = ops.softmax_xent(x, t)
    for _ in range(2):
        for r in res:
            r.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        for u, v in zip(a, res):
            assert torch.equal(u, v)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("grad_output", [1.0, 0.25])
def test_classifier_loss_through_autograd(grad_output, dtype):
    from ffwm_amd import losses
    for family, B, N in (("random", 3, 257), ("masked", 2, _chunk() + 1), ("target_is_max", 10, 79077)):
        case, bound = _case_and_bound(B, N, family, dtype)
        x = case.logits.to(DEV).requires_grad_(True)
        crit = losses.ClassifierLoss(fused=True)
        loss = crit(x, case.target.to(DEV))
        (loss * grad_output).backward()
        assert crit.prec1.is_cuda and crit.prec1.shape == () and crit.prec5.shape == () and int(crit.skipped) == 0
        out = torch.stack((loss.detach(), crit.prec1, crit.prec5))
        bound.check(out=out, rank=crit.rank, grad=x.grad, grad_output=grad_output, what="module x%g" % grad_output)
    # non-contiguous logits and other dtypes take the composition
    crit = losses.ClassifierLoss(fused=True)
    case, bound = _case_and_bound(3, 257, "random", torch.float32)
    wide = torch.zeros(3, 514, device=DEV)
    wide[:, ::2] = case.logits.to(DEV)
    loss = crit(wide[:, ::2], case.target.to(DEV))
    assert crit.rank is None and abs(float(loss) - bound.out0) <= 1e-5 * abs(bound.out0)
    loss = crit(case.logits.to(DEV).half(), case.target.to(DEV))
    assert crit.rank is None and loss.dtype == torch.float16


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_precisions_equal_the_reference_accuracy(dtype):
    """On the `random` family (no two logits of a row equal) topk's order is defined: accuracy() restated gives the same percentages."""
    for B, N in xb.shapes(_chunk()):
        case, bound = _case_and_bound(B, N, "random", dtype)
        if N < 5:
            continue                       # accuracy()'s topk(5) needs five classes
        out = _call(case, want_grad=False)[0]
        want = xb.reference_accuracy(case.logits.to(DEV), case.target.to(DEV))
        # accuracy() counts in float32 whatever the logits' dtype (correct_k.float() times the rounded 100 / B): two float32 roundings
        assert [float(out[1]), float(out[2])] == pytest.approx(want, rel=4 * xb.U32, abs=0), (B, N)

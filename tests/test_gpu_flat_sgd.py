"""The flat SGD step on the GPU (csrc/sgd.hip): ffwm_sgd_step against the per-element float64 bounds of tests/sgd_bounds.py on every
case, with NaN guard cells around all three arrays; optim.FlatSGD over a small module with the four group kinds against
torch.optim.SGD in float64; a learning rate changed through param_groups reaching a captured, replayed step; the parameters staying
views under unchanged state_dict names."""
import os
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgd_bounds as sb  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = sb.cases()


def _run(case, steps):
    from ffwm_amd import _lib
    lib = _lib.load()
    pw, p = sb.guarded(case.p.to(DEV))
    bw, buf = sb.guarded(case.buf.to(DEV))
    seg_end = torch.tensor(case.seg_end, dtype=torch.int64, device=DEV)
    seg_group = torch.tensor(case.seg_group, dtype=torch.int32, device=DEV)
    lr = torch.tensor([g[0] for g in case.groups], dtype=torch.float64, device=DEV)
    wd = torch.tensor([g[1] for g in case.groups], dtype=torch.float64, device=DEV)
    for k in range(steps):
        gw, g = sb.guarded(case.grads[k].to(DEV))
        _lib.check(lib.ffwm_sgd_step(p.data_ptr(), g.data_ptr(), buf.data_ptr(), case.n, seg_end.data_ptr(), seg_group.data_ptr(),
                                     len(case.seg_end), lr.data_ptr(), wd.data_ptr(), len(case.groups), case.momentum, _lib.F32,
                                     torch.cuda.current_stream().cuda_stream), "ffwm_sgd_step")
        torch.cuda.synchronize()
        assert sb.guards_intact(gw) and torch.equal(g.cpu(), case.grads[k]), "the gradient array was written"
    assert sb.guards_intact(pw) and sb.guards_intact(bw), "a write outside params or the momentum buffer"
    return p, buf


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_entry_point_meets_the_bounds(case):
    bound = sb.Bound(case)
    for steps in (1, 3):
        p, buf = _run(case, steps)
        bound.check(p, buf, steps, what="kernel")


class _Small(nn.Module):
    """The four group kinds of lightcnn/finetune.py:74-86 with sizes that are no multiples of 4."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 5, 3)          # 135 + 5
        self.fc = nn.Linear(7, 3)               # 21 + 3
        self.fc2 = nn.Linear(3, 11)             # 33 + 11


def _groups(net, lr=1e-2, wd=1e-3):
    out = []
    for name, value in net.named_parameters():
        if "bias" in name:
            out.append({"params": value, "lr": (20 if "fc2" in name else 2) * lr, "weight_decay": 0})
        else:
            out.append({"params": value, "lr": (10 if "fc2" in name else 1) * lr, "weight_decay": wd})
    return out


def _flat(net, capturable=False):
    from ffwm_amd.dp import BucketedGradReducer
    from ffwm_amd.optim import FlatSGD
    red = BucketedGradReducer(list(net.parameters()), gather=False)
    return red, FlatSGD(_groups(net), red, momentum=0.9, capturable=capturable)


def test_flat_sgd_against_torch_sgd_in_float64():
    torch.manual_seed(3)
    net = _Small().to(DEV)
    names = list(net.state_dict())
    ref = _Small().double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in net.state_dict().items()})
    red, opt = _flat(net)
    assert len(opt.param_groups) == 6 and list(net.state_dict()) == names
    for p in net.parameters():          # views of the one flat array
        assert opt.params.data_ptr() <= p.data_ptr() < opt.params.data_ptr() + 4 * opt.n and getattr(p, "_ffwm_flat_adam", False)
    assert int(opt.seg_group.max()) == 3          # four settings -> four device groups
    ropt = torch.optim.SGD(_groups(ref), lr=1.0, momentum=0.9)
    gen = torch.Generator().manual_seed(9)
    for step in range(3):
        opt.zero_grad()
        assert float(red.flat.abs().max()) == 0
        for p, q in zip(net.parameters(), ref.parameters()):
            g = torch.randn(p.shape, generator=gen)
            p.grad.copy_(g)
            q.grad = g.double()
        opt.step()
        ropt.step()
    torch.cuda.synchronize()
    for (k, p), q in zip(net.named_parameters(), ref.parameters()):
        # three steps of five roundings each on values of at most max|q|, and the gradient sums behind them: 64 u is far above it
        assert float((p.detach().cpu().double() - q.detach()).abs().max()) <= 64 * sb.U32 * float(q.detach().abs().max()), k
    assert list(net.state_dict()) == names


def test_a_changed_rate_reaches_a_replayed_step():
    torch.manual_seed(4)
    net = _Small().to(DEV)
    red, opt = _flat(net, capturable=True)
    gen = torch.Generator().manual_seed(2)
    for p in net.parameters():
        p.grad.copy_(torch.randn(p.shape, generator=gen))
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        opt.step()
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        opt.step()
    torch.cuda.synchronize()
    before = opt.params.clone()
    for group in opt.param_groups:
        group["lr"] = 0.0
    opt.sync_lr()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(opt.params, before), "a replay with every rate at 0.0 moved the parameters"
    buf = opt.momentum_buf.clone()
    opt.param_groups[0]["lr"] = 0.5               # conv.weight alone
    opt.sync_lr()
    g.replay()
    torch.cuda.synchronize()
    a, b = red.offset[net.conv.weight]
    moved = opt.params != before
    assert bool(moved[a - opt.lo:b - opt.lo].any()) and not bool(moved[b - opt.lo:].any()) and not bool(moved[:a - opt.lo].any())
    want = before[a - opt.lo:b - opt.lo].double() - 0.5 * opt.momentum_buf[a - opt.lo:b - opt.lo].double()
    assert float((opt.params[a - opt.lo:b - opt.lo].double() - want).abs().max()) <= 4 * sb.U32 * float(want.abs().max())
    assert not torch.equal(buf, opt.momentum_buf)

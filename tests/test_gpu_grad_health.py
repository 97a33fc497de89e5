"""Gradient health on the GPU: ffwm_grad_health on every case of tests/grad_health_cases.py (bounds, untouched inputs and guard cells,
the workspace query, bit-equal repeats, the refusals); ffwm_adam_step_guarded against ffwm_adam_step_device bit for bit (clean, one
NaN, clipped); FlatAdam's guarded step captured and replayed with the decision taken on the device; both trainers, eager, with a NaN
pixel in the input -- an input value, not a fault: nothing here is meant to make the GPU fault."""
import copy
import math
import os
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_health_cases as gh  # noqa: E402
import step_bounds as sb  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = gh.cases()
LR, B1, B2, EPS = 2e-4, 0.5, 0.999, 1e-8


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from ffwm_amd import _lib as L
    return L, L.load()


def _health(lib_mod, lib, g, n, seg_end, ws, ws_bytes, rec):
    lib_mod.check(lib.ffwm_grad_health(g.data_ptr(), n, seg_end.data_ptr(), seg_end.numel(), ws.data_ptr(), ws_bytes, rec.data_ptr(),
                                       lib_mod.F32, _stream()), "ffwm_grad_health")


# ------------------------------------------------------------------------------------------------ the entry point
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_entry_point_meets_the_bounds(case):
    L, lib = _lib()
    n, n_seg = case.n, len(case.seg_end)
    g = sb.guarded(case.g, DEV)                                   # NaN cells behind element n - 1: a read past the end would be counted
    seg_end = torch.tensor(case.seg_end, dtype=torch.int64, device=DEV)
    ws_bytes = lib.ffwm_grad_health_workspace_bytes(n, n_seg)
    assert ws_bytes > 0 and ws_bytes % 32 == 0
    ws = sb.guarded_nan(ws_bytes // 8, torch.float64, DEV)        # exactly what the query asks for, guard cells behind it
    rec = sb.guarded_nan(4 * n_seg, torch.float64, DEV)
    _health(L, lib, g, n, seg_end, ws, ws_bytes, rec)
    torch.cuda.synchronize()
    gh.check_record(case, rec)
    assert torch.equal(sb.bits(g[:n]), sb.bits(case.g)), "the gradient array was written"
    sb.check_guards(g, n, "grads")
    sb.check_guards(ws, ws_bytes // 8, "workspace")
    sb.check_guards(rec, 4 * n_seg, "record")
    # a second call, into a workspace that holds other leftovers: the same bits
    ws2 = torch.full((ws_bytes // 8,), 7.0, dtype=torch.float64, device=DEV)
    rec2 = sb.guarded_nan(4 * n_seg, torch.float64, DEV)
    _health(L, lib, g, n, seg_end, ws2, ws_bytes, rec2)
    torch.cuda.synchronize()
    assert torch.equal(sb.bits(rec2), sb.bits(rec)), "two calls differ"


def test_entry_point_refusals():
    L, lib = _lib()
    g = torch.zeros(1032, device=DEV)
    ws = torch.zeros(1024, dtype=torch.float64, device=DEV)
    rec = torch.zeros(4 * 17, dtype=torch.float64, device=DEV)

    def call(gp, n, ends, n_seg=None, ws_bytes=8192):
        t = torch.tensor(ends, dtype=torch.int64, device=DEV)
        return lib.ffwm_grad_health(gp, n, t.data_ptr(), len(ends) if n_seg is None else n_seg, ws.data_ptr(), ws_bytes, rec.data_ptr(),
                                    L.F32, _stream())
    assert call(g.data_ptr(), 1027, [516, 1027]) == 0
    assert call(g.data_ptr() + 4, 1027, [1027]) == -1 and b"aligned" in lib.ffwm_last_error()
    assert call(g.data_ptr(), 1027, list(range(4, 68, 4)) + [1027]) == -1 and b"n_seg" in lib.ffwm_last_error()          # seventeen
    assert call(g.data_ptr(), 1027, [5, 1027]) == -1 and b"multiple of 4" in lib.ffwm_last_error()
    assert call(g.data_ptr(), 1027, [516, 1024]) == -1 and b"n = 1027" in lib.ffwm_last_error()                           # the last end is not n
    assert call(g.data_ptr(), 1027, [516, 512, 1027]) == -1 and b"ascending" in lib.ffwm_last_error()
    assert call(g.data_ptr(), 1027, [1027], ws_bytes=16) == -1 and b"workspace" in lib.ffwm_last_error()
    torch.cuda.synchronize()
    from ffwm_amd import ops
    rec = ops.grad_health(g[:1027], [516, 1027])
    assert rec.shape == (2, 4) and rec.tolist() == [[0.0, 0.0, 0.0, 516.0], [0.0, 0.0, 0.0, 511.0]]


# ------------------------------------------------------------------------------------------------ the guarded step
class _Arrays:
    """p, g, m, v (guarded copies on the device), the 4-double state, and for the guarded entry the health buffers and the guard."""

    def __init__(self, p, g, m, v):
        self.n = p.numel()
        self.p, self.g, self.m, self.v = (sb.guarded(t, DEV) for t in (p, g, m, v))
        self.state = torch.tensor([0.0, 0.0, 0.0, -1.0], dtype=torch.float64, device=DEV)
        self.seg_end = torch.tensor([self.n], dtype=torch.int64, device=DEV)
        self.rec = torch.zeros(4, dtype=torch.float64, device=DEV)
        self.guard = torch.zeros(6, dtype=torch.float64, device=DEV)
        L, lib = _lib()
        self.ws_bytes = lib.ffwm_grad_health_workspace_bytes(self.n, 1)
        self.ws = torch.empty(self.ws_bytes // 8, dtype=torch.float64, device=DEV)

    def set_grad(self, g):
        self.g[:self.n] = g.to(DEV)

    def plain(self):
        L, lib = _lib()
        L.check(lib.ffwm_adam_step_device(self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n, LR, B1, B2,
                                          EPS, self.state.data_ptr(), L.F32, _stream()), "ffwm_adam_step_device")
        torch.cuda.synchronize()

    def guarded(self, max_norm=0.0, skip=1):
        L, lib = _lib()
        _health(L, lib, self.g, self.n, self.seg_end, self.ws, self.ws_bytes, self.rec)
        L.check(lib.ffwm_adam_step_guarded(self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n, LR, B1,
                                           B2, EPS, self.state.data_ptr(), self.rec.data_ptr(), 1, max_norm, skip,
                                           self.guard.data_ptr(), L.F32, _stream()), "ffwm_adam_step_guarded")
        torch.cuda.synchronize()

    def same(self, other, what):
        for name in ("p", "m", "v", "state"):
            a, b = getattr(self, name), getattr(other, name)
            assert torch.equal(sb.bits(a), sb.bits(b)), "%s: %s differs" % (what, name)          # (the guard cells with them)


@pytest.mark.parametrize("n", [5, 1027, sb.ADAM_BIG])
def test_guarded_step_on_clean_gradients_is_the_device_step(n):
    p, g, m, v, _ = sb.adam_inputs(n)
    a, b = _Arrays(p, g, m, v), _Arrays(p, g, m, v)
    for step in (1, 2):
        a.plain()
        b.guarded()
        b.same(a, "step %d" % step)
        assert b.guard.tolist()[:4] == [0.0, 1.0, 0.0, float(step)] and b.guard[5].item() == 0
    assert torch.equal(sb.bits(b.g[:n]), sb.bits(g)), "the gradient array was written"
    for arr in (b.p, b.g, b.m, b.v):
        sb.check_guards(arr, n, "guarded step")


def test_guarded_step_skips_a_nan_and_goes_on_as_if_it_had_not_been():
    n = 1027
    p, g, m, v, _ = sb.adam_inputs(n, seed=1)
    bad = g.clone()
    bad[3] = sb.NAN
    a, b, start = _Arrays(p, g, m, v), _Arrays(p, bad, m, v), _Arrays(p, g, m, v)
    b.guarded()
    b.same(start, "skipped call")                                   # params, moments and the whole state, bit for bit
    total = b.rec[0].item()
    assert b.guard.tolist() == [1.0, 0.0, 1.0, 1.0, total, 1.0] and total > 0
    b.set_grad(g)
    b.guarded()
    a.plain()                                                       # step 1 from the same arrays
    b.same(a, "the clean call behind the skipped one")
    assert b.guard.tolist()[:4] == [0.0, 1.0, 1.0, 2.0] and b.state[0].item() == 1.0
    # without skip_nonfinite the same gradients go through, as they do in ffwm_adam_step_device
    c, d = _Arrays(p, bad, m, v), _Arrays(p, bad, m, v)
    c.guarded(skip=0)
    d.plain()
    c.same(d, "skip_nonfinite off")
    assert c.guard.tolist()[:4] == [0.0, 1.0, 0.0, 1.0] and c.guard[5].item() == 1.0


def test_clip_is_the_device_step_on_prescaled_gradients():
    from ffwm_amd.optim import clip_coefficient
    n = 1027
    p, _, m, v, _ = sb.adam_inputs(n, seed=2)
    g = (torch.randn(n, generator=torch.Generator().manual_seed(5)) * 0.1)
    norm = float(g.double().norm())
    assert norm > 2.0
    b = _Arrays(p, g, m, v)
    b.guarded(max_norm=1.0)
    scale = b.guard[1].item()
    want = clip_coefficient(b.rec[0].item(), 1.0)
    print("GRADHEALTH clip: norm %.9g scale %.9g clip_coefficient %.17g" % (norm, scale, want))
    assert scale == sb.f32(scale) and abs(scale - want) <= sb.ulp32(want) and 0.3 < scale < 0.5
    a = _Arrays(p, g * torch.tensor(scale, dtype=torch.float32), m, v)
    a.plain()
    b.same(a, "clipped")
    assert torch.equal(sb.bits(b.g[:n]), sb.bits(g)), "the gradient array was rescaled in memory"
    # below the limit: exactly 1, and the plain step
    c, d = _Arrays(p, g, m, v), _Arrays(p, g, m, v)
    c.guarded(max_norm=100.0)
    d.plain()
    assert c.guard[1].item() == 1.0
    c.same(d, "norm below max_norm")


# ------------------------------------------------------------------------------------------------ FlatAdam, captured
class _Small(nn.Module):
    """Sizes that are no multiples of 4 (tests/test_gpu_flat_sgd.py)."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 5, 3)          # 135 + 5
        self.fc = nn.Linear(7, 3)               # 21 + 3
        self.fc2 = nn.Linear(3, 11)             # 33 + 11


def _flat(net, **kw):
    from ffwm_amd.dp import BucketedGradReducer
    from ffwm_amd.optim import FlatAdam
    red = BucketedGradReducer(list(net.parameters()), gather=False)
    return red, FlatAdam(list(net.parameters()), red, lr=1e-2, betas=(B1, B2), capturable=True, **kw)


def test_default_flat_adam_allocates_nothing_new():
    net = _Small().to(DEV)
    _, opt = _flat(net)
    assert not opt.guarded and opt.record is None and opt.guard is None and opt.workspace is None and opt.seg_end is None
    with pytest.raises(RuntimeError):
        opt.health()


def test_captured_step_decides_on_the_device():
    from ffwm_amd import graphs
    torch.manual_seed(6)
    net = _Small().to(DEV)
    twin = copy.deepcopy(net)
    segs = [("fc2", list(net.fc2.parameters())), ("fc", list(net.fc.parameters())), ("conv", list(net.conv.parameters()))]
    red, opt = _flat(net, monitor=True, skip_nonfinite=True, max_grad_norm=1e9, segments=segs)
    red2, ref = _flat(twin)
    gen = torch.Generator().manual_seed(8)
    pad = torch.ones(red.flat.numel(), dtype=torch.bool)
    for q in net.parameters():
        a, b = red.offset[q]
        pad[a:b] = False
    # (padding elements stay zero, as the reducer keeps them)
    clean = [torch.where(pad, torch.zeros(pad.numel()), torch.randn(pad.numel(), generator=gen)).to(DEV) for _ in range(2)]
    poisoned = clean[0].clone()
    poisoned[red.offset[net.fc.weight][0] + 2] = math.inf
    # warm-up outside the capture, on zero gradients: parameters and moments stay as they are, the step counters of both move to 1
    graphs.warm_up(opt.step, 1, DEV, sync=True)
    graphs.warm_up(ref.step, 1, DEV, sync=True)
    graph, _ = graphs.capture(opt.step)
    seen = []
    for grads in (clean[0], poisoned, clean[1]):
        red.flat.copy_(grads)
        graph.replay()
        torch.cuda.synchronize()
        seen.append(opt.health())
    assert [h["skipped"] for h in seen] == [False, True, False]
    assert [h["steps_applied"] for h in seen] == [2, 2, 3] and [h["steps_seen"] for h in seen] == [2, 3, 4]
    assert seen[2]["steps_skipped"] == 1 and [h["scale"] for h in seen] == [1.0, 0.0, 1.0]
    assert [seen[1][k]["nonfinite"] for k in ("fc2", "fc", "conv")] == [0, 1, 0] and seen[0]["fc"]["nonfinite"] == 0
    a = 0
    for k, end in opt.segments:          # a segment ends where the next network's first parameter begins, the last one at the last element
        assert end == (red.offset[{"fc2": net.fc.bias, "fc": net.conv.bias}[k]][0] if k != "conv" else red.offset[net.conv.weight][1])
        want, m = float(clean[1][a:end].double().norm()), end - a
        # the kernel's sum and torch's float64 sum: m u each, halved by the square root; two square roots
        assert seen[2][k]["n"] == m and abs(seen[2][k]["norm"] - want) <= (m + 2) * gh.U64 * want
        a = end
    for grads in clean:
        red2.flat.copy_(grads)
        ref.step()
    torch.cuda.synchronize()
    assert torch.equal(sb.bits(opt.params), sb.bits(ref.params)), "applied, skipped, applied is not two plain steps"
    assert torch.equal(sb.bits(opt.exp_avg), sb.bits(ref.exp_avg)) and torch.equal(sb.bits(opt.exp_avg_sq), sb.bits(ref.exp_avg_sq))
    assert torch.equal(sb.bits(opt.state[:3]), sb.bits(ref.state[:3]))


# ------------------------------------------------------------------------------------------------ the trainers, eager
def _optimizers(t):
    return [(k, getattr(t, k)) for k in ("opt_F", "opt_G", "opt_D", "optimizer") if hasattr(t, k)]


def _check_trainer(t, batch):
    t.step(batch)
    torch.cuda.synchronize()
    h = t.health()
    for label, opt in _optimizers(t):
        assert h[label]["skipped"] is False and h[label]["steps_applied"] == 1 and h[label]["scale"] == 1.0
        a = 0
        for name, end in opt.segments:
            x = opt.reducer.flat[opt.lo + a:opt.lo + end].double()
            want, m = float(x.norm()), end - a
            # the kernel's sum and torch's float64 sum: m u each, halved by the square root; two square roots
            print("GRADHEALTH %s %s: norm %.17g float64 %.17g n %d" % (type(t).__name__, name, h[name]["norm"], want, m))
            assert want > 0 and abs(h[name]["norm"] - want) <= (m + 2) * gh.U64 * want
            assert h[name]["n"] == m and h[name]["nonfinite"] == 0 and h[name]["max_abs"] == float(x.abs().max())
            a = end
    before = {label: (opt.params.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.state[:3].clone()) for label, opt in _optimizers(t)}
    bad = dict(batch)
    bad["img_S"] = batch["img_S"].clone()
    bad["img_S"][0, 1, 40, 50] = math.nan
    t.step(bad)
    torch.cuda.synchronize()
    h = t.health()
    for label, opt in _optimizers(t):
        assert h[label]["skipped"] is True and h[label]["steps_skipped"] == 1 and h[label]["steps_seen"] == 2, (label, h[label])
        assert sum(h[name]["nonfinite"] for name, _ in opt.segments) > 0
        for was, now in zip(before[label], (opt.params, opt.exp_avg, opt.exp_avg_sq, opt.state[:3])):
            assert torch.equal(sb.bits(was), sb.bits(now)), "%s: a skipped step changed the optimizer" % label


def test_flownet_trainer_reports_and_skips():
    from ffwm_amd import trainer
    t = trainer.FlowNetTrainer(DEV, ngf=8, grad_health=True, skip_nonfinite=True)
    assert [name for name, _ in t.optimizer.segments] == ["flowNet"]
    _check_trainer(t, trainer.synthetic_batch(2, DEV))


def test_ffwm_trainer_reports_and_skips():
    from ffwm_amd import trainer
    t = trainer.FFWMTrainer(DEV, ngf=4, grad_health=True, skip_nonfinite=True)
    assert sorted(name for name, _ in t.opt_F.segments) == ["flowNetB", "flowNetF"]
    assert [name for name, _ in t.opt_G.segments] == ["netG"] and [name for name, _ in t.opt_D.segments] == ["netD"]
    _check_trainer(t, trainer.synthetic_batch(2, DEV))
    assert set(t.health()) == {"flowNetF", "flowNetB", "netG", "netD", "opt_F", "opt_G", "opt_D"}

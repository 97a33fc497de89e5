"""The fused BatchNorm kernels (csrc/bn_lrelu.hip) against the per-channel yardstick of tests/bn_bounds.py, straight through the C
ABI so that the test picks the route by passing or withholding scratch: four entry points x wave / block / split shapes x float4 /
scalar path x LeakyReLU / sigmoid, input families mixed across the channels, a NaN / inf channel, and an exact +-1 family bit for
bit.  Every output is pre-filled with NaN (every element must be written), per-channel arrays carry 16 NaN guard cells, the scratch
must be zero again after every call, wave and block routes are bit-identical from run to run.  Run with ``-m gpu`` on the MI355X.

``python tests/test_gpu_bn_bounds.py --report profiles/bn_bounds.txt`` writes the worst error / bound per entry point, route, path and
family of the same matrix."""
import functools
import os
import sys

import pytest
import torch

import bn_bounds as bb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")


def _p(t):
    return None if t is None else t.data_ptr()


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _guarded(C, init=None):
    a = bb.guarded(C, device=DEV)
    if init is not None:
        a[:C] = init.to(DEV)
    return a


def _new_scratch(name):
    C = bb.SHAPES[name][0][1]
    return torch.zeros(bb.scratch_doubles(C), device=DEV, dtype=torch.float64) if bb.SHAPES[name][1] else None


def _scratch_is_zero(scratch):
    """Sums and arrival counters: every byte."""
    return scratch is None or torch.equal(scratch.view(torch.int64), torch.zeros_like(scratch, dtype=torch.int64))


def call_forward(case, scratch):
    """-> y, save_mean, save_invstd, running_mean, running_var on the device (NaN-filled outputs, guarded per-channel arrays)."""
    from ffwm_amd import _lib
    lib = _lib.load()
    B, C, H, W = case.shape
    x, w, b = _dev(case.x), _dev(case.gamma), _dev(case.beta)
    rm = None if case.run_mean is None else _guarded(C, case.run_mean)
    rv = None if case.run_var is None else _guarded(C, case.run_var)
    y = torch.full(case.shape, NAN, device=DEV)
    sm, si = _guarded(C), _guarded(C)
    if case.variant == "plain":
        rc = lib.ffwm_bn_lrelu_forward(_p(x), _p(w), _p(b), _p(rm), _p(rv), _p(y), _p(sm), _p(si), _p(scratch), B, C, H * W, case.eps,
                                       case.momentum, case.slope, _lib.F32, _stream())
        _lib.check(rc, "ffwm_bn_lrelu_forward")
    else:
        res, rbias = _dev(case.res), _dev(case.rbias)
        rc = lib.ffwm_bn_res_act_forward(_p(x), _p(w), _p(b), _p(rm), _p(rv), _p(res), _p(rbias), _p(y), _p(sm), _p(si), _p(scratch), B, C,
                                         H * W, case.eps, case.momentum, case.slope, case.act, _lib.F32, _stream())
        _lib.check(rc, "ffwm_bn_res_act_forward")
    torch.cuda.synchronize()
    return y, sm, si, rm, rv


def call_backward(bc, scratch):
    """-> dx, d(gamma), d(beta), d(res) (None for the plain variant)."""
    from ffwm_amd import _lib
    lib = _lib.load()
    B, C, H, W = bc.shape
    x, dy, w, b = _dev(bc.x), _dev(bc.dy), _dev(bc.gamma), _dev(bc.beta)
    sm, si = _dev(bc.save_mean), _dev(bc.save_invstd)
    dx = torch.full(bc.shape, NAN, device=DEV)
    dw, db = _guarded(C), _guarded(C)
    dres = None
    if bc.variant == "plain":
        rc = lib.ffwm_bn_lrelu_backward(_p(x), _p(dy), _p(w), _p(b), _p(sm), _p(si), _p(dx), _p(dw), _p(db), _p(scratch), B, C, H * W,
                                        bc.slope, _lib.F32, _stream())
        _lib.check(rc, "ffwm_bn_lrelu_backward")
    else:
        y = _dev(bc.y)
        dres = torch.full(bc.shape, NAN, device=DEV)
        rc = lib.ffwm_bn_res_act_backward(_p(x), _p(y), _p(dy), _p(w), _p(sm), _p(si), _p(dx), _p(dres), _p(dw), _p(db), _p(scratch), B, C,
                                          H * W, bc.slope, bc.act, _lib.F32, _stream())
        _lib.check(rc, "ffwm_bn_res_act_backward")
    torch.cuda.synchronize()
    return dx, dw, db, dres


def _same(a, b):
    """Bit-identical, NaNs included."""
    if a is None:
        return b is None
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@functools.lru_cache(maxsize=2)
def _prepared(spec, exact):
    """The case, its route and both bounds: built once, shared by the forward and the backward test of the case, never modified.
    The backward entry is given the REFERENCE's float statistics and output, so its test does not lean on the forward kernel."""
    case, route = (bb.build_exact if exact else bb.build_mixed)(spec)
    fb = bb.ForwardBound(case, route)
    bc = bb.backward_inputs(case, fb.mean.float(), fb.invstd.float(), fb.ref.float() if case.variant == "res" else None)
    return case, route, fb, bc, bb.BackwardBound(bc, route)


def run_forward(spec, exact=False):
    case, route, fb, _, _ = _prepared(spec, exact)
    scratch = _new_scratch(spec[0])
    out = call_forward(case, scratch)
    assert _scratch_is_zero(scratch), "scratch not zero after the call (%s)" % route
    fam = fb.check(*out)
    if route.kind != "split":                       # no atomics: the same bits every time
        again = call_forward(case, scratch)
        assert all(_same(a, b) for a, b in zip(out, again)), "two runs differ on the %s route" % route.kind
        assert _scratch_is_zero(scratch)
    return route, fam


def run_backward(spec, exact=False):
    case, route, _, bc, bwd = _prepared(spec, exact)
    scratch = _new_scratch(spec[0])
    out = call_backward(bc, scratch)
    assert _scratch_is_zero(scratch), "scratch not zero after the call (%s)" % route
    fam = bwd.check(*out, exact_dx=bool(exact and spec[-1]))
    if route.kind != "split":
        again = call_backward(bc, scratch)
        assert all(_same(a, b) for a, b in zip(out, again)), "two runs differ on the %s route" % route.kind
    return route, fam


RUN = {"forward": run_forward, "backward": run_backward}


@pytest.mark.parametrize("spec,direction", [pytest.param(s, d, id=bb.case_id(s) + "-" + d) for s in bb.mixed_cases() for d in RUN])
def test_entry_points_meet_the_bounds(spec, direction):
    RUN[direction](spec)


@pytest.mark.parametrize("spec,direction", [pytest.param(s, d, id="-".join(str(v) for v in s) + "-" + d) for s in bb.exact_cases() for d in RUN])
def test_entry_points_are_exact_on_the_exact_family(spec, direction):
    RUN[direction](spec, exact=True)


SPLIT = [n for n, s in bb.SHAPES.items() if s[2] == "split"]


@pytest.mark.parametrize("name,variant,nonfinite", [pytest.param(n, v, f, id="%s-%s-%s" % (n, v, "nonfinite" if f else "finite")) for n in SPLIT
                                                    for v in bb.VARIANTS for f in (False, True) if not f or bb.SHAPES[n][0][1] >= 2])
def test_one_scratch_buffer_serves_forward_backward_and_forward_again(name, variant, nonfinite):
    """The caller's contract: ONE buffer, zero-filled once; after every call it is zero again -- also with a NaN channel, whose sums
    are NaN in the scratch until the last reader clears them."""
    spec = (name, variant, "a", 0, nonfinite)
    case, route, fb, bc, bwd = _prepared(spec, False)
    assert route.kind == "split" and route.S >= 2
    scratch = _new_scratch(name)
    fb.check(*call_forward(case, scratch))
    assert _scratch_is_zero(scratch)
    bwd.check(*call_backward(bc, scratch))
    assert _scratch_is_zero(scratch)
    fb.check(*call_forward(case, scratch))
    assert _scratch_is_zero(scratch)


# ------------------------------------------------------------------------------------------------ the module layer
LAYER_SHAPE = "split_mid_plane"


def _settled(variant):
    """A case whose plain-variant mask is unambiguous under its OWN statistics (the module layer computes them from the x it is given):
    nudge, recompute the statistics, until no element lies within 3 margins of the kink."""
    res, act = bb.VARIANTS[variant]
    case = bb.make_case(bb.SHAPES[LAYER_SHAPE][0], res, act, "a", 0)
    route = bb.route_of(LAYER_SHAPE)
    for _ in range(8):
        fb = bb.ForwardBound(case, route)
        mean_f, invstd_f = fb.mean.float(), fb.invstd.float()
        if variant != "plain" or not bool(bb.ambiguous(case.x, case.gamma, case.beta, mean_f, invstd_f, 3.0).any()):
            return case, route, fb
        g, b, xhat, xabs, pre, margin, free = bb._pre_margin(case.x, case.gamma, case.beta, mean_f, invstd_f)
        amb = bb.ambiguous(case.x, case.gamma, case.beta, mean_f, invstd_f, 3.0)
        step = 12 * margin / (g.abs() * invstd_f.double()).view(1, -1, 1, 1).expand_as(pre)
        away = torch.where(pre >= 0, 1.0, -1.0) * torch.sign(g).view(1, -1, 1, 1).expand_as(pre)
        case.x = torch.where(amb, (case.x.double() + away * step).float(), case.x).contiguous()
    raise AssertionError("the kink could not be cleared")


def _layer(variant, apply):
    """apply(x, w, b, rm, rv, res, rbias, case) -> y with autograd; the saved statistics are read off the graph's saved tensors."""
    case, route, fb = _settled(variant)
    C = case.shape[1]
    x = _dev(case.x).requires_grad_(True)
    w, b = torch.nn.Parameter(_dev(case.gamma)), torch.nn.Parameter(_dev(case.beta))
    rm, rv = _dev(case.run_mean), _dev(case.run_var)
    res = None if case.res is None else _dev(case.res).requires_grad_(True)
    rbias = None if case.rbias is None else _dev(case.rbias).requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        y = apply(x, w, b, rm, rv, res, rbias, case)
    # saved in this order by all three layers: ..., weight (, bias), save_mean, save_invstd (, y)
    stats = [t for t in saved if tuple(t.shape) == (C,) and t.data_ptr() not in (w.data_ptr(), b.data_ptr())]
    assert len(stats) == 2, [tuple(t.shape) for t in saved]
    fb.check(y.detach(), stats[0], stats[1], rm, rv)
    bc = bb.backward_inputs(case, stats[0], stats[1], y.detach() if variant != "plain" else None)
    assert torch.equal(bc.x, case.x)                       # already off the kink: nothing left to nudge
    bwd = bb.BackwardBound(bc, route)
    y.backward(_dev(bc.dy))
    torch.cuda.synchronize()
    bwd.check(x.grad, w.grad, b.grad, None if res is None else res.grad)
    if rbias is not None:
        assert torch.equal(rbias.grad, b.grad)             # one sum serves both


def _one_zero_scratch():
    from ffwm_amd import norm
    return len(norm._SCRATCH) == 1 and all(_scratch_is_zero(s) for s in norm._SCRATCH.values())


def test_python_function_layer_hands_the_kernel_what_the_abi_tests_do():
    from ffwm_amd import norm
    norm.reset_scratch()
    _layer("plain", lambda x, w, b, rm, rv, res, rbias, c: norm._BnLreluFunction.apply(x, w, b, rm, rv, c.eps, c.momentum, c.slope))
    assert _one_zero_scratch()                             # the cache handed out a buffer (the split route) and got it back zero


def test_cpp_binding_layer_hands_the_kernel_what_the_abi_tests_do():
    from ffwm_amd import _ext
    ext = _ext.get()
    if ext is None:
        pytest.skip("the C++ autograd binding is not built")
    _layer("plain", lambda x, w, b, rm, rv, res, rbias, c: ext.bn_lrelu(x, w, b, rm, rv, c.eps, c.momentum, c.slope))


@pytest.mark.parametrize("variant", ["res_lrelu", "res_sigmoid"])
def test_residual_tail_layer_hands_the_kernel_what_the_abi_tests_do(variant):
    import torch.nn as nn
    from ffwm_amd import norm
    norm.reset_scratch()
    made = []

    def apply(x, w, b, rm, rv, res, rbias, c):
        bn = nn.BatchNorm2d(x.shape[1], eps=c.eps, momentum=c.momentum).to(DEV).train()
        bn.weight, bn.bias = w, b
        bn.running_mean, bn.running_var = rm, rv
        made.append(bn)
        assert norm.bn_res_act_ok(bn, x, c.act)
        return norm.bn_res_act(x, bn, res, rbias, c.act, c.slope)
    _layer(variant, apply)
    assert _one_zero_scratch() and int(made[0].num_batches_tracked) == 1


# ------------------------------------------------------------------------------------------------ the record
def _report(path):
    rows, ran = {}, set()
    for spec in bb.mixed_cases():
        for direction, run in RUN.items():
            route, fam = run(spec)
            entry = ("ffwm_bn_lrelu_" if spec[1] == "plain" else "ffwm_bn_res_act_") + direction
            ran.add((entry, route.kind, route.path))
            for f, v in fam.items():
                key = (entry, route.kind, route.path, f)
                rows[key] = max(rows.get(key, 0.0), v)
    for spec in bb.exact_cases():
        for direction, run in RUN.items():
            route, fam = run(spec, exact=True)
            entry = ("ffwm_bn_lrelu_" if spec[1] == "plain" else "ffwm_bn_res_act_") + direction
            key = (entry, route.kind, route.path, "exact")
            rows[key] = max(rows.get(key, 0.0), max(fam.values()))
    lines = ["# worst |got - ref| / bound per entry point, route, path and input family (tests/bn_bounds.py, SAFETY = %g);" % bb.SAFETY,
             "# exact: 0 = bit for bit.  Written by `python tests/test_gpu_bn_bounds.py --report` on %s." % torch.cuda.get_device_name(0),
             "%-28s %-6s %-7s %-9s %s" % ("entry", "route", "path", "family", "error/bound")]
    for (entry, kind, path_, f), v in sorted(rows.items()):
        lines.append("%-28s %-6s %-7s %-9s %.4f" % (entry, kind, path_, f, v))
    worst = max(rows.values())
    lines.append("# worst of all: %.4f; (entry, route, path) combinations run: %d" % (worst, len(ran)))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if worst <= 1.0 else 1


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if len(sys.argv) == 3 and sys.argv[1] == "--report":
        sys.exit(_report(sys.argv[2]))
    sys.exit("usage: test_gpu_bn_bounds.py --report FILE")

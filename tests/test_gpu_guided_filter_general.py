"""GuidedFilter beyond FFWM's own call: planes of any size, a one-channel guide, the gradient for y.

Oracle: ``ffwm_amd.nets.GuidedFilter(r)`` -- the restatement that tests/test_nets_golden.py pins to the reference's output -- on the
CPU in float64 with autograd on x and y; inputs uniform [0, 1) from a seeded generator.  r >= 1 throughout (r = 0 makes var_x = 0
against eps = 1e-8, where the reference's own fp32 result is off by 50 x scale).

Bounds: the project's guided-filter tolerance (tests/test_gpu_parity.py) 2e-4 in fp32 and 1e-9 in fp64, as
``max|got - ref| <= tol (1 + max|ref|)`` for the output and the sharper ``<= tol max|ref|`` for the gradients (max|grad_x| is only
0.03-0.2 on these inputs).  The fp32 restatement's own distance from float64 is printed next to every fp32 figure."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = {torch.float32: 2e-4, torch.float64: 1e-9}

CASES = [
    # (B, Cx, Cy, H, W, r)
    (1, 1, 1, 9, 129, 3),        # one past the line limit of the four-launch kernels in W only; smallest H for r = 3
    (1, 2, 2, 130, 12, 5),       # one past the limit in H only
    (1, 1, 1, 4, 260, 1),        # minimal r and H; a row of two chunks
    (1, 2, 2, 200, 136, 66),     # window 133 of a 136-wide line: crosses every segment and chunk boundary
    (2, 3, 3, 160, 257, 20),     # ragged in both directions; several planes
    (1, 3, 3, 512, 512, 32),     # power-of-two sizes
    (1, 1, 1, 1030, 520, 7),     # long lines, short window
    (2, 1, 3, 64, 48, 8),        # one-channel guide on the <= 128 geometry
    (1, 1, 2, 150, 140, 16),     # one-channel guide on long lines
    (1, 3, 3, 128, 128, 32),     # FFWM's geometry, now also with grad_y
]
COMBO_CASES = [(2, 3, 3, 160, 257, 20), (2, 1, 3, 64, 48, 8)]


@functools.lru_cache(maxsize=None)
def _inputs(case):
    B, Cx, Cy, H, W, r = case
    g = torch.Generator().manual_seed(1000 + H * 7 + W * 3 + r + Cx + B)
    x = torch.rand(B, Cx, H, W, generator=g, dtype=torch.float64)
    y = torch.rand(B, Cy, H, W, generator=g, dtype=torch.float64)
    go = torch.rand(B, Cy, H, W, generator=g, dtype=torch.float64)
    return x, y, go


def _restatement(case, dtype):
    from ffwm_amd import nets
    x, y, go = (t.to(dtype) for t in _inputs(case))
    xr, yr = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    out = nets.GuidedFilter(case[5])(xr, yr)
    out.backward(go)
    return out.detach().double(), xr.grad.double(), yr.grad.double()


@functools.lru_cache(maxsize=None)
def _oracle(case):
    """(out, grad_x, grad_y) in float64 on the CPU: computed once per case, shared, never modified."""
    return _restatement(case, torch.float64)


@functools.lru_cache(maxsize=None)
def _restatement_fp32_distance(case):
    return tuple((a - b).abs().max().item() for a, b in zip(_restatement(case, torch.float32), _oracle(case)))


def _hip(case, dtype, need_x=True, need_y=True):
    from ffwm_amd.external_function import GuidedFilter
    x, y, go = (t.to(DEV, dtype) for t in _inputs(case))
    x.requires_grad_(need_x)
    y.requires_grad_(need_y)
    out = GuidedFilter(case[5])(x, y)
    if need_x or need_y:
        out.backward(go)
    return out.detach(), x.grad, y.grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_matches_float64_restatement(case, dtype):
    ref = _oracle(case)
    got = [t.cpu().double() for t in _hip(case, dtype)]
    tol = TOL[dtype]
    dist = [(g - r).abs().max().item() for g, r in zip(got, ref)]
    scale = [r.abs().max().item() for r in ref]
    bound = [tol * (1 + scale[0]), tol * scale[1], tol * scale[2]]
    line = "guided filter %s %s:" % (case, str(dtype).split(".")[1])
    for name, d, s in zip(("out", "grad_x", "grad_y"), dist, scale):
        line += "  %s hip %.2e of max|ref|" % (name, d / s)
    if dtype == torch.float32:
        line += "  | fp32 restatement: " + " ".join("%.2e" % (d / s) for d, s in zip(_restatement_fp32_distance(case), scale))
    print(line)
    for name, g, r, d, b in zip(("out", "grad_x", "grad_y"), got, ref, dist, bound):
        assert g.shape == r.shape, name
        assert d <= b, "%s: max abs diff %.3e > %.3e" % (name, d, b)       # NaN (poisoned memory read) fails too
        assert torch.isfinite(g).all(), name


@pytest.mark.parametrize("case", COMBO_CASES, ids=lambda c: "x".join(map(str, c)))
def test_only_the_gradients_asked_for(case):
    """ctx.needs_input_grad: the gradient nobody asked for is None, the other has the bits of the both-gradients run."""
    out, gx, gy = _hip(case, torch.float32)
    out_x, gx_only, none_y = _hip(case, torch.float32, True, False)
    out_y, none_x, gy_only = _hip(case, torch.float32, False, True)
    out_0, n0, n1 = _hip(case, torch.float32, False, False)
    assert none_y is None and none_x is None and n0 is None and n1 is None
    assert torch.equal(gx_only, gx) and torch.equal(gy_only, gy)
    assert torch.equal(out_x, out) and torch.equal(out_y, out) and torch.equal(out_0, out)


def test_bit_identical_from_run_to_run():
    case = (2, 1, 3, 150, 140, 16)
    a, b = _hip(case, torch.float32), _hip(case, torch.float32)
    for s, t in zip(a, b):
        assert torch.equal(s, t)
    ref = _oracle(case)
    assert (a[1].cpu().double() - ref[1]).abs().max().item() <= 2e-4 * ref[1].abs().max().item()


def test_graph_capture_replays_the_eager_bits():
    from ffwm_amd import ops
    case = (2, 3, 3, 160, 257, 20)
    x, y, go = (t.to(DEV, torch.float32) for t in _inputs(case))
    r = case[5]

    def step():
        out, saved = ops.guided_filter_forward(x, y, r)
        gx, gy = ops.guided_filter_backward_xy(x, y, saved, go, r, True, True)
        return out, gx, gy

    eager = [t.clone() for t in step()]                      # also the warm-up: the library is loaded, the allocator primed
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step()
    for _ in range(2):
        for t in held:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(held, eager):
            assert torch.equal(got, want)


def test_contract():
    from ffwm_amd import _lib, ops
    from ffwm_amd.external_function import GuidedFilter
    with pytest.raises(AssertionError):                      # c_x = 2, c_y = 3: the reference's assertion
        GuidedFilter(3)(torch.rand(1, 2, 16, 16, device=DEV), torch.rand(1, 3, 16, 16, device=DEV))
    big = torch.rand(1, 1, 4, 8200, device=DEV)              # beyond the documented 8192 per side
    with pytest.raises(_lib.FFWMError, match=r"status -3.*8192"):
        GuidedFilter(1)(big, big)
    x = torch.rand(1, 1, 201, 300, device=DEV)
    with pytest.raises(AssertionError):
        GuidedFilter(100)(x, x)                              # H = 2r+1
    with pytest.raises(_lib.FFWMError, match=r"status -1.*2r\+1"):
        ops.guided_filter_forward(x, x, 100)

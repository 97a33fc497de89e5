"""The scatter backward kernels against the per-cell yardstick of tests/scatter_bounds.py: every cell within
rho sum|w g| + eta L of the float64 reference (L: the channel's largest gradient within reach of the cell), non-finite cells
exactly where the reference has them.  A matrix of operator x kernel path x input family; every path is asserted to have run
through its profiler scope, every option is restored in `finally`.  Sizes are those at which the default production path
serves the call (resample2d's owned tiles from 2^18 pixels).  Run with ``-m gpu`` on the MI355X."""
import contextlib
import functools

import pytest
import torch

import scatter_bounds as sb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DEFAULTS = {"rs_bwd1_owned": 0, "rs_bwd1_fixed": 0, "scatter_variant": 0, "be_bwd_fixed": 0, "warp_feat_fixed": 0,
            "ba_bwd_fused": 3, "ba_bwd_pix": 4}


@contextlib.contextmanager
def _scoped(options):
    """Set `options`, profile what runs inside, restore the defaults; yields the dict the scopes are collected into."""
    from ffwm_amd import _lib
    rows = {}
    try:
        for k, v in options.items():
            _lib.set_option(k, v)
        _lib.prof_reset()
        _lib.prof_enable(True)
        yield rows
        torch.cuda.synchronize()
        rows.update(_lib.prof_collect())
    finally:
        _lib.prof_enable(False)
        for k in options:
            _lib.set_option(k, DEFAULTS[k])


def _assert_ran(rows, scope):
    assert any(k.startswith(scope) for k in rows), (scope, sorted(rows))


# ------------------------------------------------------------------------------------------------ resample2d d_input1
RS_FAMILIES = sb.FAMILIES + ("small_sigma",)
# path: (options, (B, C, H, W), ks, dtype, scope)
RS_PATHS = {
    "owned": ({}, (1, 8, 512, 512), 4, torch.float32, "resample2d_bwd_input1_owned"),
    "owned_ks2": ({}, (1, 8, 512, 512), 2, torch.float32, "resample2d_bwd_input1_owned"),
    "tile_fixed": ({"rs_bwd1_owned": 2}, (1, 8, 512, 512), 4, torch.float32, "resample2d_bwd_input1_tile"),
    "tile_pair_double": ({"rs_bwd1_owned": 2, "rs_bwd1_fixed": 2}, (1, 8, 512, 512), 4, torch.float32, "resample2d_bwd_input1_auto"),
    "taplane": ({}, (1, 8, 256, 256), 4, torch.float32, "resample2d_bwd_input1_taplane"),
    "plane": ({}, (1, 8, 96, 120), 2, torch.float32, "resample2d_bwd_input1_plane"),
    "fp64": ({}, (1, 8, 96, 120), 4, torch.float64, "resample2d_bwd_input1_plane"),
}


@functools.lru_cache(maxsize=None)
def _rs_case(kind, shape, ks, dtype):
    B, C, H, W = shape
    in2 = sb.rs_small_sigma(B, H, W, 31) if kind == "small_sigma" else sb.rs_flow(B, H, W, 30)
    go = sb.family_grad("signed" if kind == "small_sigma" else kind, shape, 32)
    return in2, go, sb.resample2d_bound(shape, in2, go, ks, dtype=dtype)


@pytest.mark.parametrize("path", list(RS_PATHS))
@pytest.mark.parametrize("kind", RS_FAMILIES)
def test_resample2d_grad_input1_per_cell(oracle, kind, path):
    from ffwm_amd import ops
    options, shape, ks, dtype, scope = RS_PATHS[path]
    in2, go, bound = _rs_case(kind, shape, ks, dtype)
    in1 = torch.zeros(shape, dtype=dtype, device=DEV)
    g1 = torch.full(shape, float("nan"), dtype=dtype, device=DEV)          # overwrite mode: every cell must be written
    with _scoped(options) as rows:
        ops.resample2d_backward(in1, in2.to(DEV, dtype), go.to(DEV, dtype), ks, 1, g1, None, overwrite_input1=True)
    _assert_ran(rows, scope)
    bound.check(g1, what="resample2d %s %s" % (path, kind))


# ------------------------------------------------------------------------------------------------ block extractor d_source
# path: (options, (B, C, Hs, Ws) = flow grid, flow reach, scope)
BE_PATHS = {
    "tile2_fixed": ({}, (1, 8, 150, 200), 2.0, "block_extractor_bwd_tile2"),
    "tile2_double": ({"be_bwd_fixed": 2}, (1, 8, 150, 200), 2.0, "block_extractor_bwd_tile2"),
    "small_plane": ({}, (1, 8, 60, 70), 2.0, "block_extractor_bwd_src_plane"),
    "far": ({}, (1, 8, 150, 200), 24.0, "block_extractor_bwd_far"),
}


@functools.lru_cache(maxsize=None)
def _be_case(kind, shape, reach):
    B, C, H, W = shape
    flow = sb.block_flow(B, H, W, 40, reach)
    go = sb.family_grad(kind, (B, C, 3 * H, 3 * W), 41)
    return flow, go, sb.block_extractor_bound(shape, flow, go, 3)


@pytest.mark.parametrize("path", list(BE_PATHS))
@pytest.mark.parametrize("kind", sb.FAMILIES)
def test_block_extractor_grad_source_per_cell(oracle, kind, path):
    from ffwm_amd import ops
    options, shape, reach, scope = BE_PATHS[path]
    flow, go, bound = _be_case(kind, shape, reach)
    gs = torch.zeros(shape, device=DEV)
    with _scoped(options) as rows:
        ops.block_extractor_backward(torch.zeros(shape, device=DEV), flow.to(DEV), go.to(DEV), 3, gs, None)
    _assert_ran(rows, scope)
    bound.check(gs, what="block_extractor %s %s" % (path, kind))


# ------------------------------------------------------------------------------------------------ block attention d_source
@functools.lru_cache(maxsize=None)
def _ba_case(kind):
    B, C, H, W = 1, 8, 100, 140
    flow = sb.block_flow(B, H, W, 50)
    w = torch.randn(B, 9, H, W, generator=torch.Generator().manual_seed(51))
    go = sb.family_grad(kind, (B, C, H, W), 52)
    return (B, C, H, W), flow, w, go, sb.block_attention_bound((B, C, H, W), flow, w, go, 3)


@pytest.mark.parametrize("fused", [1, 2, 3])
@pytest.mark.parametrize("kind", sb.FAMILIES)
def test_block_attention_grad_source_per_cell(oracle, kind, fused):
    """The default ba_bwd_src route (fused = 3) and the other ba_bwd_fused variants of test_block_attention_backward_by_linearity."""
    from ffwm_amd import ops
    shape, flow, w, go, bound = _ba_case(kind)
    gs = torch.zeros(shape, device=DEV)
    with _scoped({"ba_bwd_fused": fused}) as rows:
        ops.block_attention_backward(torch.zeros(shape, device=DEV), flow.to(DEV), w.to(DEV), go.to(DEV), 3, gs, None, None)
    _assert_ran(rows, "block_attention_bwd_src")
    bound.check(gs, what="block attention fused %d %s" % (fused, kind))


# ------------------------------------------------------------------------------------------------ warp d_feat
@functools.lru_cache(maxsize=None)
def _warp_case(kind):
    B, C, H, W = 1, 8, 256, 256
    flow = sb.warp_grid(B, H, W, 60)
    go = sb.family_grad(kind, (B, C, H, W), 61)
    return (B, C, H, W), flow, go, sb.warp_bound((B, C, H, W), flow, go)


@pytest.mark.parametrize("fixed", [0, 1, 3, 4])
@pytest.mark.parametrize("kind", sb.FAMILIES)
def test_warp_grad_feat_per_cell(oracle, kind, fixed):
    """warp_feat_fixed 0: the default double cells; 1 / 3 / 4: the fixed-point cell variants."""
    from ffwm_amd import ops
    shape, flow, go, bound = _warp_case(kind)
    gf = torch.full(shape, float("nan"), device=DEV)
    with _scoped({"warp_feat_fixed": fixed}) as rows:
        ops.warp_backward(torch.zeros(shape, device=DEV), flow.to(DEV), go.to(DEV), False, gf, None, overwrite_feat=True)
    _assert_ran(rows, "warp_bwd_feat_tile")
    bound.check(gf, what="warp fixed %d %s" % (fixed, kind))


# ------------------------------------------------------------------------------------------------ empty flow grids
def _nan_block_freed(n, dtype):
    """Leave a NaN-filled block of n elements in the caching allocator: the next allocation of that size reuses it."""
    t = torch.full((n,), float("nan"), dtype=dtype, device=DEV)
    torch.cuda.synchronize()
    del t


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_resample2d_function_empty_flow_grid_returns_zero_gradient(dtype):
    from ffwm_amd.external_function import Resample2dFunction
    in1 = torch.rand(2, 3, 20, 24, dtype=dtype, device=DEV, requires_grad=True)
    in2 = torch.zeros(2, 3, 0, 24, dtype=dtype, device=DEV, requires_grad=True)
    out = Resample2dFunction.apply(in1, in2, 4, 1)
    assert out.shape == (2, 3, 0, 24)
    _nan_block_freed(in1.numel(), dtype)
    out.sum().backward()
    assert in1.grad is not None and torch.equal(in1.grad, torch.zeros_like(in1))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_warp_function_empty_flow_grid_returns_zero_gradient(dtype):
    from ffwm_amd.external_function import WarpFunction
    feat = torch.rand(2, 3, 20, 24, dtype=dtype, device=DEV, requires_grad=True)
    flow = torch.zeros(2, 2, 0, 24, dtype=dtype, device=DEV, requires_grad=True)
    out = WarpFunction.apply(feat, flow, False)
    assert out.shape == (2, 3, 0, 24)
    _nan_block_freed(feat.numel(), dtype)
    out.sum().backward()
    assert feat.grad is not None and torch.equal(feat.grad, torch.zeros_like(feat))

"""The gather backward kernels against the per-pixel yardstick of tests/gather_bounds.py: every element of resample2d's d_input2, the
block extractor's d_flow, block attention's d_flow / d_weights and the warp's d_flow within rho x (the sum of the absolute values of
its terms) + kappa of the float64 reference, rho from the case's channel and tap count, non-finite elements exactly where the
reference has them.  A matrix of operator x kernel path x input family; every path is asserted to have run through its profiler
scope and every option is restored in `finally`.  The shapes are the smallest that reach each arm (tests/gather_bounds.py holds
them: the float32 oracle is checked against the same bounds at the same shapes in tests/test_gather_bounds_cpu.py).

The two warp d_flow kernels -- warp_bwd_flow_lds_kernel and warp_bwd_kernel -- share one profiler scope (`warp_bwd_flow@H`; the
benchmark keys on it), so they are told apart by forcing the route: warp_fwd_variant = 2 sends a d_flow-alone call to the LDS
kernel, 1 to the direct kernel; the one case of exactly 2^24 pixel-channels reaches the LDS kernel by the default route.
Each test prints its error / bound (``-s`` shows them).  Run with ``-m gpu`` on the MI355X.

rho is a worst-case figure, linear in taps x C, so it leaves the more slack the more channels a case has: on the 2^24 route
(C = 64, rho about 1050 u) the kernel sits at 0.003 of its bound, and that case would only notice an error a few hundred times the
kernel's real one -- it is there for the route, the 128-bit loads and the slabs, not as a tight check; the few-channel cases are.

Worst error / bound measured on the MI355X, and in brackets the float32 oracle's at the same rho (no kernel sits nearer its bound
than the reference does):

    resample2d d_input2         lds 0.023, pixel / generic 0.011, float64 0.027      (0.039)
    block extractor d_flow      pixel / generic 0.012, tiles 0.003, float64 0.006     (0.014)
    block attention d_flow      0.003, float64 0.007                                  (0.008)
    block attention d_weights   0.036, float64 0.033                                  (0.044)
    warp d_flow, power-of-two sizes (kappa = 0): lds 0.054, 2^24 route 0.003, slab of 5 (four-channel loop, pair loads) 0.016   (0.054)
    warp d_flow, other sizes: lds 0.55 (launches with direct-gather tiles 0.35), direct 0.53, shared 0.37, multi 0.33, float64 0.032    (0.55)
  (on sizes that are no power of two the fp32 rounding of ix, iy -- kappa -- is the error, and the kernels round the coordinates as the
   oracle does: kernel and float32 oracle give the same 0.554 on the same pixel of in [1, 3, 96, 130] -> grid 80 x 129)"""
import contextlib

import pytest
import torch

import gather_bounds as gb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DEFAULTS = {"scatter_variant": 0, "warp_fwd_variant": 0, "be_bwd_variant": 0, "be_bwd_fixed": 0, "ba_bwd_pix": 4}


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


def _ran(rows, scope):
    """The scope itself, or the scope with its size suffix (`warp_bwd_flow@64`) -- not a longer name that starts with it."""
    return any(k == scope or k.startswith(scope + "@") for k in rows)


def _assert_ran(rows, *scopes):
    for scope in scopes:
        assert _ran(rows, scope), (scope, sorted(rows))


def _report(what, ratio):
    print("RATIO %s %.3f" % (what, ratio))


# ------------------------------------------------------------------------------------------------ resample2d d_input2
RS_PATHS = {name: ({"scatter_variant": 2} if name == "pixels_sv2" else {},
                   "resample2d_bwd_input2_lds" if name.startswith("lds") else "resample2d_bwd_input2") for name in gb.RS_CASES}


def _rs_run(name, in1, in2, go):
    from ffwm_amd import ops
    _, _, ks, dil, _, _, dtype = gb.RS_CASES[name]
    options, scope = RS_PATHS[name]
    g2 = torch.full(in2.shape, float("nan"), dtype=dtype, device=DEV)      # the operator overwrites: every element must be written
    with _scoped(options) as rows:
        ops.resample2d_backward(in1.to(DEV, dtype), in2.to(DEV, dtype), go.to(DEV, dtype), ks, dil, None, g2)
    _assert_ran(rows, scope)
    assert not _ran(rows, "resample2d_bwd_input2" if scope.endswith("lds") else "resample2d_bwd_input2_lds"), sorted(rows)
    return g2


@pytest.mark.parametrize("kind", gb.FAMILIES)
@pytest.mark.parametrize("name", list(gb.RS_CASES))
def test_resample2d_grad_input2_per_pixel(oracle, name, kind):
    in1, in2, go, bound = gb.rs_case(name, kind)
    g2 = _rs_run(name, in1, in2, go)
    _report("resample2d %s %s" % (name, kind), bound.check(g2, what="resample2d %s %s" % (name, kind)))


@pytest.mark.parametrize("name", ["lds_fallback", "lds_c6", "pixels_dil2"])
def test_resample2d_grad_input2_nonfinite_flow_pixels(oracle, name):
    """One flow pixel of 1e30 and one of NaN (a block that meets either leaves the LDS box for direct gathers): non-finite results
    sit where the reference has them, and every other pixel still meets its bound."""
    in1, in2, go, bound = gb.rs_case(name, "signed")
    ks, dil = gb.RS_CASES[name][2:4]
    bad = in2.clone()
    bad[0, 0, 5, 7] = 1e30
    bad[0, 1, 9, 11] = float("nan")
    _, ref = oracle.resample2d_backward(in1.double(), bad.double(), go.double(), ks, dil)
    g2 = _rs_run(name, in1, bad, go).cpu()
    assert gb.same_nonfinite(g2, ref) == 0 and not bool(torch.isfinite(ref[0, :, 9, 11]).any())
    for y, x in ((5, 7), (9, 11)):
        g2[0, :, y, x] = bound.ref[0, :, y, x].to(g2.dtype)
    bound.check(g2, what="resample2d %s, the other pixels" % name)


# ------------------------------------------------------------------------------------------------ block extractor d_flow
# (case, options, scopes that must have run)
BE_PATHS = {
    "pixels": ("pixels", {}, ("block_extractor_bwd", "block_extractor_bwd_src_plane")),     # the plane route takes d_source
    "pixels_f64": ("pixels_f64", {}, ("block_extractor_bwd", "block_extractor_bwd_src_plane")),
    "pixels_k2": ("pixels_k2", {}, ("block_extractor_bwd",)),
    "pixels_k4": ("pixels_k4", {}, ("block_extractor_bwd",)),
    "pixels_k5": ("pixels_k5", {}, ("block_extractor_bwd",)),
    "pixels_k5_f64": ("pixels_k5_f64", {}, ("block_extractor_bwd",)),
    "grids": ("grids", {}, ("block_extractor_bwd",)),
    "generic_k9": ("generic_k9", {}, ("block_extractor_bwd_generic",)),
    "tile2_fixed": ("tiles", {}, ("block_extractor_bwd_tile2",)),
    "tile2_double": ("tiles", {"be_bwd_fixed": 2}, ("block_extractor_bwd_tile2",)),
    "tile2_far": ("tiles_far", {}, ("block_extractor_bwd_tile2", "block_extractor_bwd_far")),
    "tile_owned": ("tiles", {"be_bwd_variant": 2}, ("block_extractor_bwd_tile",)),
    "tile_owned_far": ("tiles_far", {"be_bwd_variant": 2}, ("block_extractor_bwd_tile", "block_extractor_bwd_far")),
}


@pytest.mark.parametrize("kind", gb.FAMILIES)
@pytest.mark.parametrize("path", list(BE_PATHS))
def test_block_extractor_grad_flow_per_pixel(oracle, path, kind):
    from ffwm_amd import ops
    name, options, scopes = BE_PATHS[path]
    dtype = gb.BE_CASES[name][4]
    src, flow, go, k, bound = gb.be_case(name, kind)
    gs = torch.zeros(src.shape, dtype=dtype, device=DEV)                   # d_source is wanted too: that is what routes the call
    gf = torch.zeros(flow.shape, dtype=dtype, device=DEV)
    with _scoped(options) as rows:
        ops.block_extractor_backward(src.to(DEV, dtype), flow.to(DEV, dtype), go.to(DEV, dtype), k, gs, gf)
    _assert_ran(rows, *scopes)
    _report("block_extractor %s %s" % (path, kind), bound.check(gf, what="block extractor %s %s" % (path, kind)))


# ------------------------------------------------------------------------------------------------ block attention d_flow, d_weights
BA_ROWS = ([("c8", pix, kind) for pix in range(6) for kind in gb.FAMILIES] + [("c6", pix, "signed") for pix in range(6)] +
           [("c6", 4, kind) for kind in gb.FAMILIES[1:]] + [("c6_f64", 4, kind) for kind in gb.FAMILIES])


@pytest.mark.parametrize("name,pix,kind", BA_ROWS)
def test_block_attention_grad_flow_and_weights_per_pixel(oracle, name, pix, kind):
    """Every ba_bwd_pix configuration of ba_bwd_pix_kernel (the call wants no d_source: the pixel kernel runs alone); float64 takes
    ba_bwd_generic, which produces all three gradients."""
    from ffwm_amd import ops
    dtype = gb.BA_CASES[name][1]
    src, flow, w, go, flow_bound, weights_bound = gb.ba_case(name, kind)
    generic = dtype == torch.float64
    gs = torch.zeros(src.shape, dtype=dtype, device=DEV) if generic else None
    gf = torch.zeros(flow.shape, dtype=dtype, device=DEV)
    gw = torch.zeros(w.shape, dtype=dtype, device=DEV)
    with _scoped({"ba_bwd_pix": pix}) as rows:
        ops.block_attention_backward(src.to(DEV, dtype), flow.to(DEV, dtype), w.to(DEV, dtype), go.to(DEV, dtype), 3, gs, gf, gw)
    _assert_ran(rows, "block_attention_bwd_generic" if generic else "block_attention_bwd_pix")
    assert generic or not _ran(rows, "block_attention_bwd_src"), sorted(rows)
    what = "block attention %s pix %d %s" % (name, pix, kind)
    _report("block_attention_flow %s pix%d %s" % (name, pix, kind), flow_bound.check(gf, what=what + " d_flow"))
    _report("block_attention_weights %s pix%d %s" % (name, pix, kind), weights_bound.check(gw, what=what + " d_weights"))


# ------------------------------------------------------------------------------------------------ warp d_flow
# path: (cases, options).  lds / direct force the kernel (see the module docstring); default leaves the route to the shape.
# Which ARM runs inside a kernel is a property of the input, proven on the CPU (tests/test_gather_bounds_cpu.py): under the zoom25
# grid some tiles of the LDS kernel exceed its 128 x 32 box and gather directly, under every other grid none does (zoom18 included);
# `slab5` is the one direct case whose plan keeps >= 4 channels per block (5: the four-channel loop and the tail), all others run
# the one-channel tail loop alone.
WARP_PATHS = {
    "lds": (("b2c5_64", "ragged_w", "grids", "slabs", "c2_66"), {"warp_fwd_variant": 2}),
    "natural": (("natural",), {}),
    "direct": (("small", "ragged", "crop", "small_f64", "ragged_f64", "slab5"), {"warp_fwd_variant": 1}),
    "default": (("small", "crop"), {}),
}
WARP_ROWS = [(path, name) + row for path, (names, _) in WARP_PATHS.items() for name in names
             for row in (gb.warp_matrix(name) if path != "default" else gb.warp_matrix(name)[:6])]


def _warp_scope(flipcat, tail="_bwd_flow"):
    return ("warp_flipcat" if flipcat else "warp") + tail


def _dead_pixels_are_zero(bound, got, grid_kind):
    if grid_kind in ("outside", "zoom18", "zoom25"):     # four invalid corners: d_flow is exactly 0 (the bound is 0 there as well)
        dead = bound.mag == 0
        assert int(dead.sum()) > 0 and float(got.detach().cpu().double()[dead].abs().max()) == 0.0


@pytest.mark.parametrize("path,name,grid_kind,kind,flipcat", WARP_ROWS)
def test_warp_grad_flow_per_pixel(oracle, path, name, grid_kind, kind, flipcat):
    from ffwm_amd import ops
    dtype = gb.WARP_CASES[name][2]
    feat, grid, go, bound = gb.warp_case(name, grid_kind, kind, flipcat)
    gl = torch.zeros(grid.shape, dtype=dtype, device=DEV)
    with _scoped(WARP_PATHS[path][1]) as rows:
        ops.warp_backward(feat.to(DEV, dtype), grid.to(DEV, dtype), go.to(DEV, dtype), flipcat, None, gl)
    _assert_ran(rows, _warp_scope(flipcat))
    what = "warp %s %s %s %s flipcat %d" % (path, name, grid_kind, kind, flipcat)
    _report(what, bound.check(gl, what=what))
    _dead_pixels_are_zero(bound, gl, grid_kind)


@pytest.mark.parametrize("flipcat", [False, True])
@pytest.mark.parametrize("grid_kind", gb.WARP_GRIDS)
def test_warp_grad_flow_from_the_shared_pixel_kernel(oracle, grid_kind, flipcat):
    """scatter_variant = 1 with both gradients wanted: ONE warp_bwd_kernel launch scatters d_feat and gathers d_flow."""
    from ffwm_amd import ops
    feat, grid, go, bound = gb.warp_case("ragged", grid_kind, "signed", flipcat)
    gf = torch.zeros(feat.shape, device=DEV)
    gl = torch.zeros(grid.shape, device=DEV)
    with _scoped({"scatter_variant": 1}) as rows:
        ops.warp_backward(feat.to(DEV), grid.to(DEV), go.to(DEV), flipcat, gf, gl)
    _assert_ran(rows, _warp_scope(flipcat, "_bwd"))
    assert not _ran(rows, _warp_scope(flipcat)), sorted(rows)
    _report("warp shared %s flipcat %d" % (grid_kind, flipcat), bound.check(gl, what="warp, shared pixel kernel, %s" % grid_kind))
    _dead_pixels_are_zero(bound, gl, grid_kind)


@pytest.mark.parametrize("flipcat", [False, True])
def test_warp_grad_flow_lds_dead_pixels_beside_a_nonfinite_cell(oracle, flipcat):
    """warp_bwd_flow_lds_kernel on the forward yardstick's input (tests/sample_forward_bounds.py): under the `outside` grid of
    in [1, 3, 96, 130] -> 80 x 129 a tile holds pixels without a valid corner and its staged box starts on a NaN cell.  Those pixels'
    d_flow is 0 as the reference's (the kernel used to add 0 x NaN), the pixels that sample a non-finite cell are non-finite, and
    every other pixel meets its bound."""
    import sample_forward_bounds as sf
    from ffwm_amd import ops
    feat, grid, _ = sf.warp_case("grids", "outside", "nonfinite", flipcat)
    go = gb.grads("signed", (1, 6 if flipcat else 3, 80, 129), 163)
    bound = gb.warp_flow_bound(feat, grid, go, flipcat)
    gl = torch.zeros(grid.shape, device=DEV)
    with _scoped({"warp_fwd_variant": 2}) as rows:
        ops.warp_backward(feat.to(DEV), grid.to(DEV), go.to(DEV), flipcat, None, gl)
    _assert_ran(rows, _warp_scope(flipcat))
    what = "warp lds, nonfinite features, flipcat %d" % flipcat
    _report(what, bound.check(gl, what=what))
    _dead_pixels_are_zero(bound, gl, "outside")


MULTI = ("multi_wide", "multi_crop", "slab5")


@pytest.mark.parametrize("kind,flipcat", [("signed", False), ("group_mags", True)])
@pytest.mark.parametrize("grid_kind", ["interior", "border"])
def test_warp_multi_grad_flow_per_pixel(oracle, grid_kind, kind, flipcat):
    """warp_bwd_flow_multi_kernel, three problems in one launch.  The pair-load arm walks a block's slab four channels per trip, so
    it needs a slab of >= 4: the launch plans [2, 8, 64, 192] and [2, 3, 64, 64] -> 16 x 16 down to ONE channel per block (96 and 8
    tiles against the 4096 blocks asked for), which is the tail loop; [4, 20, 256, 256] keeps 5 (gb.warp_pixel_slab: 1024 tiles x 4
    slabs = 4096) -- one pair-load trip and one tail channel.  Under `interior` every pixel has its four corners inside the image,
    so every wave is whole and takes the pair loads; under `border` the waves at the image's edge take the dword loop instead."""
    from ffwm_amd import ops
    assert gb.warp_pixel_slab(4, 20, 256, 256) == 5
    cases = [gb.warp_case(name, grid_kind, kind, flipcat) for name in MULTI]
    gls = [torch.zeros(c[1].shape, device=DEV) for c in cases]
    with _scoped({}) as rows:
        ops.warp_multi_backward([c[0].to(DEV) for c in cases], [c[1].to(DEV) for c in cases], [c[2].to(DEV) for c in cases], flipcat,
                                [None] * len(cases), gls)
    _assert_ran(rows, _warp_scope(flipcat, "_bwd_flow_multi"))
    for name, c, gl in zip(MULTI, cases, gls):
        what = "warp multi %s %s %s flipcat %d" % (name, grid_kind, kind, flipcat)
        _report(what, c[3].check(gl, what=what))

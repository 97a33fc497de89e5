"""The forward kernels of the sampling operators against the per-element yardstick of tests/sample_forward_bounds.py: every element
of the warp's, resample2d's, the block extractor's and block attention's output within rho x (the same forward of |source|) + kappa
of the float64 reference, NaN and +-Inf exactly where the reference has them, and bit for bit the float64 reference on the exact
family.  A matrix of operator x kernel route x input family; the float32 oracle is held to the same bounds at the same shapes in
tests/test_sample_forward_bounds_cpu.py.

Every call writes into a NaN-prefilled `out=` destination (an unwritten element shows), runs twice and must agree with itself bit
for bit (the forwards use no atomics), is asserted to have taken its route through the profiler scopes, and restores every option
in `finally`.  Kernels that share a scope are told apart by forcing the route:
  * warp_fwd_kernel and warp_fwd_lds_kernel share `warp_fwd@H` / `warp_flipcat_fwd@H`: warp_fwd_variant = 1 / 2 forces either; the
    one case of exactly 2^24 elements reaches the LDS kernel by the default route.  Which tiles of the LDS kernel leave LDS, and
    which direct cases keep a four-channel slab, are properties of the inputs proven on the CPU.
  * ba_fwd_pix_kernel (ba_fwd_pix = 1 .. 4) and be_fwd_lds_kernel's attention mode (0) share `block_attention_fwd_lds`.
  * rs_fwd_kernel and rs_fwd_generic share `resample2d_fwd`: kernel_size 8 has no rs_fwd_kernel instance.
  * the streaming-store (nt) arms of warp_fwd_lds_kernel and be_fwd_lds_kernel are taken by outputs of >= 64 MiB: one such call
    must equal, bit for bit, the per-sample calls of the same kernel, whose outputs are below 64 MiB.
ops.warp_multi_forward allocates its own outputs, so that test fills the problem table itself to hand in NaN-prefilled ones.
Each test prints ``RATIO <what> <error / bound>`` (``-s`` shows them).  Run with ``-m gpu`` on the MI355X.

Worst error / bound measured on the MI355X, and in brackets the float32 oracle's on the same inputs at the same rho:

    warp, power-of-two sizes (kappa = 0)   direct 0.108 (four-channel trips), lds 0.098, 2^24 route 0.113, multi 0.113     (the same)
    warp, other sizes (kappa leads)        direct 0.575, lds 0.519, multi 0.575, float64 < 0.001                        (the same)
    block extractor                        lds / direct / generic 0.087, float64 < 0.001                                (0.087)
    block attention                        ba_fwd_pix 1-4 0.036, 0 0.025, generic (k = 2) 0.036, float64 < 0.001        (0.032, 0.032, 0.036)
    resample2d                             lds 0.046, direct (dilation 2) 0.046, generic 0.015, float64 0.024           (0.048, 0.046, 0.015)
    resample2d, small sigma / sigma 0.1    lds 0.044 / 0.091, direct 0.003 / 0.031, float64 0.002; sigma = 0: 0        (the same)
  The warp and extractor kernels reproduce the float32 oracle's figures to the last digit (the extractor is asserted equal to it
  element by element, on every route and family).  Two kernels sit a little nearer their bound than the reference on single
  cases, both at 3 % of it: ba_fwd_pix_kernel (0.036 against the composition's 0.032 on feat_mags sources and weights; 0.033
  against 0.026 on `masked`) contracts Wy^T (w / k^2) Wx before it meets the samples, where the composition rounds extract x w
  first and pools after -- another association of the same factors; rs_fwd_lds_kernel at kernel_size 5 (0.030 against 0.024)
  accumulates by fma in LDS order and divides by Markstein's reciprocal sequence.  Neither is a defect.

The yardstick's one finding, fixed with it: warp_fwd_lds_kernel gave a pixel WITHOUT a valid corner the first four cells of its
tile's staged box times weight 0 -- NaN, where the box starts on a non-finite cell, instead of the reference's 0 (`lds grids outside
nonfinite`: 1298 elements on the kernel as it was; the multi launch's LDS arm runs the same body; include/ffwm_hip.h states the
contract).  warp_bwd_flow_lds_kernel added the same 0 x NaN to d_flow and is fixed and tested beside it
(tests/test_gpu_gather_bounds.py::test_warp_grad_flow_lds_dead_pixels_beside_a_nonfinite_cell).
"""
import contextlib
import ctypes

import pytest
import torch

import sample_forward_bounds as sf

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DEFAULTS = {"warp_fwd_variant": 0, "be_fwd_variant": 0, "ba_fwd_pix": 1}
NAN = float("nan")


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
    """The scope itself, or the scope with its size suffix (`warp_fwd@64`) -- not a longer name that starts with it."""
    return any(k == scope or k.startswith(scope + "@") for k in rows)


def _routes(rows, ran, others=()):
    assert _ran(rows, ran), (ran, sorted(rows))
    for scope in others:
        assert scope == ran or not _ran(rows, scope), (scope, sorted(rows))


def _same_bits(a, b):
    view = torch.int32 if a.dtype == torch.float32 else torch.int64
    return torch.equal(a.view(view), b.view(view))


def _same_values(a, b):
    """Equal element by element, a NaN matching a NaN (the sign and payload of a produced NaN are the processor's)."""
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _twice(run, shape, dtype, options):
    """run(out) into two NaN-prefilled destinations under `options`: -> (the first, the scopes); the two agree bit for bit."""
    outs = [torch.full(tuple(shape), NAN, dtype=dtype, device=DEV) for _ in range(2)]
    with _scoped(options) as rows:
        for out in outs:
            run(out)
    assert _same_bits(outs[0], outs[1]), "two calls differ"
    return outs[0], rows


def _report(what, ratio):
    print("RATIO %s %.3f" % (what, ratio))


def _dev(dtype, *ts):
    return [t.to(DEV, dtype) for t in ts]


# ------------------------------------------------------------------------------------------------ warp
WARP_OPTIONS = {"direct": {"warp_fwd_variant": 1}, "lds": {"warp_fwd_variant": 2}, "natural": {}}


def _warp_scope(flipcat, tail=""):
    return ("warp_flipcat_fwd" if flipcat else "warp_fwd") + tail


def _warp_run(feat, grid, flipcat, dtype, options):
    from ffwm_amd import ops
    f, g = _dev(dtype, feat, grid)
    B, C = feat.shape[:2]
    out, rows = _twice(lambda o: ops.warp_forward(f, g, flipcat, o), (B, 2 * C if flipcat else C) + tuple(grid.shape[2:]), dtype, options)
    _routes(rows, _warp_scope(flipcat), (_warp_scope(not flipcat), _warp_scope(False, "_multi"), _warp_scope(True, "_multi")))
    return out


def _dead_pixels_are_zero(bound, got):
    dead = bound.mag == 0                   # no valid corner: exactly 0, whatever the source holds
    if int(dead.sum()):
        assert float(got.detach().cpu().double()[dead].abs().max()) == 0.0


@pytest.mark.parametrize("path,name,grid_kind,kind,flipcat", [r for r in sf.WARP_ROWS if r[0] != "multi"])
def test_warp_forward_per_element(oracle, path, name, grid_kind, kind, flipcat):
    dtype = sf.WARP_CASES[name][2]
    feat, grid, bound = sf.warp_case(name, grid_kind, kind, flipcat)
    out = _warp_run(feat, grid, flipcat, dtype, WARP_OPTIONS[path])
    what = "warp %s %s %s %s flipcat %d" % (path, name, grid_kind, kind, flipcat)
    _report(what, bound.check(out, what=what))
    _dead_pixels_are_zero(bound, out)


@pytest.mark.parametrize("flipcat", [False, True])
@pytest.mark.parametrize("shape", sf.EXACT_WARP)
@pytest.mark.parametrize("path", ["direct", "lds"])
def test_warp_forward_exact_family(oracle, path, shape, flipcat):
    """Integer sources, flows on multiples of 2^-9: every product and partial sum is exact in fp32, so the kernel equals the float64
    reference -- and the source value itself where the flow is an integer (the reference, proven on the CPU, does)."""
    feat, grid, ref = sf.warp_exact_case(shape, flipcat)
    out = _warp_run(feat, grid, flipcat, torch.float32, WARP_OPTIONS[path])
    assert torch.equal(out.cpu().double(), ref)


@pytest.mark.parametrize("flipcat", [False, True])
def test_warp_forward_streaming_stores(flipcat):
    """warp_fwd_lds_kernel with nt = 1: an output of exactly 64 MiB ([2, 32, 512, 512], or [2, 16, ..] doubled by flipcat) against
    the two per-sample calls of the same kernel (32 MiB each: plain stores)."""
    from ffwm_amd import ops
    B, C, H, W = 2, 16 if flipcat else 32, 512, 512
    feat = sf.source("feat_mags", (B, C, H, W), 270).to(DEV)
    grid = sf.warp_grid("signed", "border", B, (H, W), (H, W), 271).to(DEV)
    Co = 2 * C if flipcat else C
    assert B * Co * H * W * 4 == 64 << 20
    whole, rows = _twice(lambda o: ops.warp_forward(feat, grid, flipcat, o), (B, Co, H, W), torch.float32, {"warp_fwd_variant": 2})
    _routes(rows, _warp_scope(flipcat))
    for b in range(B):
        part, rows = _twice(lambda o: ops.warp_forward(feat[b:b + 1], grid[b:b + 1], flipcat, o), (1, Co, H, W), torch.float32,
                            {"warp_fwd_variant": 2})
        _routes(rows, _warp_scope(flipcat))
        assert _same_bits(whole[b:b + 1].contiguous(), part), b


def _warp_multi_into(feats, flows, outs, flipcat):
    """ops.warp_multi_forward with the caller's outputs (the operator allocates its own, uninitialised)."""
    from ffwm_amd import _lib, ops
    arr = ops._warp_table(feats, flows, outs=outs)
    with ops._on_device(feats[0]) as stream:
        _lib.check(_lib.load().ffwm_warp_multi_forward(ctypes.cast(arr, ctypes.c_void_p), len(feats), 1 if flipcat else 0,
                                                       ops._dtype_code(feats[0]), stream), "ffwm_warp_multi_forward")


def _multi_wants_lds(name):
    (_, C, Hi, Wi), grid_hw, dtype = sf.WARP_CASES[name]
    H, W = grid_hw or (Hi, Wi)
    return dtype == torch.float32 and H >= 32 and W >= 32 and C >= 32


@pytest.mark.parametrize("flipcat", [False, True])
def test_warp_multi_forward_per_element(oracle, flipcat):
    """Nine small problems in the table (it flushes at kMaxWarpProblems = 8: two warp_fwd_multi launches), both arms of
    multi_wants_lds among them, each output judged by its own bound; without flipcat the 2^24 problem joins, which fwd_wants_lds
    sends to warp_fwd_lds_kernel in a launch of its own."""
    picks = list(sf.MULTI) + ([sf.MULTI_ALONE] if not flipcat else [])
    cases = [sf.warp_case(name, "border", kind, flipcat) for name, kind in picks]
    assert len(sf.MULTI) == 9 and sum(_multi_wants_lds(n) for n, _ in sf.MULTI) == 3
    feats, flows = [c[0].to(DEV) for c in cases], [c[1].to(DEV) for c in cases]
    both = []
    with _scoped({}) as rows:
        for _ in range(2):
            outs = [torch.full(tuple(c[2].ref.shape), NAN, device=DEV) for c in cases]
            _warp_multi_into(feats, flows, outs, flipcat)
            both.append(outs)
    _routes(rows, _warp_scope(flipcat, "_multi"), (_warp_scope(not flipcat, "_multi"), _warp_scope(not flipcat)))
    assert _ran(rows, _warp_scope(flipcat)) == (not flipcat), sorted(rows)
    for (name, kind), c, out, again in zip(picks, cases, both[0], both[1]):
        assert _same_bits(out, again), name
        what = "warp multi %s %s flipcat %d" % (name, kind, flipcat)
        _report(what, c[2].check(out, what=what))


# ------------------------------------------------------------------------------------------------ block extractor
def _be_run(src, flow, k, dtype, options, scope):
    from ffwm_amd import ops
    s, f = _dev(dtype, src, flow)
    B, C = src.shape[:2]
    out, rows = _twice(lambda o: ops.block_extractor_forward(s, f, k, o), (B, C, k * flow.shape[2], k * flow.shape[3]), dtype, options)
    _routes(rows, scope, sf.BE_SCOPES)
    return out


@pytest.mark.parametrize("path,kind", sf.BE_ROWS)
def test_block_extractor_forward_per_element(oracle, path, kind):
    """The bound, and -- what the suite claims of the fp32 extractor (test_block_extractor_forward_is_bit_exact_fp32) -- equality
    with the float32 oracle, on every family and route."""
    name, options, scope = sf.BE_PATHS[path]
    dtype = sf.BE_CASES[name][4]
    src, flow, k, bound = sf.be_case(name, kind)
    out = _be_run(src, flow, k, dtype, options, scope)
    what = "block_extractor %s %s" % (path, kind)
    _report(what, bound.check(out, what=what))
    if dtype == torch.float32:
        assert _same_values(out.cpu(), oracle.block_extractor_forward(src, flow, k)), what + ": differs from the float32 oracle"


@pytest.mark.parametrize("name,variant", [(n, 0) for n in sf.EXACT_BE] + [("k3", 1), ("k2", 1), ("k3", 9)])
def test_block_extractor_forward_exact_family(oracle, name, variant):
    src, flow, k, ref = sf.be_exact_case(name)
    scope = ("block_extractor_fwd_generic" if variant == 9 or k > 7 else
             "block_extractor_fwd_lds" if variant == 0 and k <= 4 else "block_extractor_fwd")
    out = _be_run(src, flow, k, torch.float32, {"be_fwd_variant": variant}, scope)
    assert torch.equal(out.cpu().double(), ref)


def test_block_extractor_forward_streaming_stores():
    """be_fwd_lds_kernel with nt = 1: [4, 16, 150, 200], k = 3 writes 69 MB (>= 64 MiB) against the four per-sample calls (17 MB)."""
    from ffwm_amd import ops
    B, C, H, W, k = 4, 16, 150, 200, 3
    src = sf.source("feat_mags", (B, C, H, W), 272).to(DEV)
    flow = sf.block_flow("signed", B, H, H, W, 273, 2.0).to(DEV)
    assert B * C * k * k * H * W * 4 >= 64 << 20 > C * k * k * H * W * 4
    whole, rows = _twice(lambda o: ops.block_extractor_forward(src, flow, k, o), (B, C, k * H, k * W), torch.float32, {})
    _routes(rows, "block_extractor_fwd_lds", sf.BE_SCOPES)
    for b in range(B):
        part, rows = _twice(lambda o: ops.block_extractor_forward(src[b:b + 1], flow[b:b + 1], k, o), (1, C, k * H, k * W), torch.float32, {})
        _routes(rows, "block_extractor_fwd_lds", sf.BE_SCOPES)
        assert _same_bits(whole[b:b + 1].contiguous(), part), b


# ------------------------------------------------------------------------------------------------ block attention
BA_SCOPES = ("block_attention_fwd_lds", "block_attention_fwd_generic")


@pytest.mark.parametrize("name,pix,kind,wkind", sf.BA_ROWS)
def test_block_attention_forward_per_element(oracle, name, pix, kind, wkind):
    from ffwm_amd import ops
    _, k, dtype = sf.BA_CASES[name]
    src, flow, w, k, bound = sf.ba_case(name, kind, wkind)
    s, f, wd = _dev(dtype, src, flow, w)
    out, rows = _twice(lambda o: ops.block_attention_forward(s, f, wd, k, o), src.shape, dtype, {"ba_fwd_pix": pix})
    _routes(rows, BA_SCOPES[0] if k == 3 and dtype == torch.float32 else BA_SCOPES[1], BA_SCOPES + sf.BE_SCOPES)
    what = "block_attention %s pix%d %s %s" % (name, pix, kind, wkind)
    _report(what, bound.check(out, what=what))


# ------------------------------------------------------------------------------------------------ resample2d
RS_SCOPES = ("resample2d_fwd_lds", "resample2d_fwd")


def _rs_run(name, in1, in2):
    from ffwm_amd import ops
    _, _, ks, dil, _, _, dtype = sf.RS_CASES[name]
    a, b = _dev(dtype, in1, in2)
    out, rows = _twice(lambda o: ops.resample2d_forward(a, b, ks, dil, o), (in2.shape[0], in1.shape[1]) + tuple(in2.shape[2:]), dtype, {})
    _routes(rows, RS_SCOPES[0] if name.startswith("lds") else RS_SCOPES[1], RS_SCOPES)
    return out


@pytest.mark.parametrize("name,kind", sf.RS_ROWS)
def test_resample2d_forward_per_element(oracle, name, kind):
    in1, in2, ks, dil, bound = sf.rs_case(name, kind)
    out = _rs_run(name, in1, in2)
    what = "resample2d %s %s" % (name, kind)
    _report(what, bound.check(out, what=what))
    if bool(bound.dead.any()):             # every float product underflows: SAFE_DIV(0, 0) = 0, exactly
        assert float(out.cpu().double()[bound.dead.expand_as(bound.ref) & torch.isfinite(bound.ref)].abs().max()) == 0.0


@pytest.mark.parametrize("kind", ["signed", "feat_mags"])
def test_resample2d_forward_with_regular_and_irregular_blocks(oracle, kind):
    """One flow pixel of 3e6 (beyond 2^20) and one NaN: their blocks leave the LDS box for direct gathers, the other blocks of the
    call stay staged.  Non-finite outputs sit where the reference has them, every other pixel still meets its bound."""
    in1, in2, ks, dil, regular = sf.rs_case("lds_c6", kind)
    bad = sf.rs_irregular(in2)
    bound = sf.resample2d_bound(in1, bad, ks, dil)
    assert not bool(torch.isfinite(bound.ref[0, :, 20, 11]).any()) and bool(torch.isfinite(bound.ref[0, :, 5, 7]).all())
    keep = torch.ones_like(bound.ref, dtype=torch.bool)
    keep[0, :, 5, 7] = keep[0, :, 20, 11] = False
    assert torch.equal(bound.ref[keep], regular.ref[keep])
    _report("resample2d irregular %s" % kind, bound.check(_rs_run("lds_c6", in1, bad), what="resample2d lds_c6 %s, irregular blocks" % kind))
